"""RotatE (openea/models/semantic/rotate.py:20-144): entities are complex vectors (two fp64 tables, real and imaginary parts), a
relation is a vector of phases, and a triple is scored by dist = sum_d |h_d e^{i theta_d} - t_d| against the margin gamma
(rotate.py:61-93).  The loss divides the negatives' half by their number per positive (rotate.py:74-82),
    loss = - sum_pos log sigmoid(gamma - dist+)  -  (1 / neg_triple_num) * sum_neg log sigmoid(dist- - gamma),
which is the one place it differs from BootEA_RotatE's.  One Adam trains the three variables.

Device side: the tables and the trainer of BootEA_RotatE (rotate_trainer.py), oea_rotate_step with cfg.neg_loss_div =
neg_triple_num (csrc/rotate_step.hip), all in fp64 like the reference's variables.  Evaluation reads `re + im` of the
(row-normalised) parts without a second normalisation (rotate.py:121-137), handed to the fp32 evaluation kernels.  The epoch
loop and its printed line are BasicModel's."""
import numpy as np

from ...modules.base.initializers import init_embeddings
from ...modules.load import read as rd
from ..basic_model import BasicModel
from .rotate_trainer import ComplexEntityTable, PhaseTable, RotateTrainer
from .semantic_trainer import check_args


class RotatE(BasicModel):

    def __init__(self):
        super().__init__()
        self.pi = 3.14159265358979323846
        self.epsilon = 2.0
        self.embedding_range = None

    def init(self):
        self._check_args()
        if self._dist_group() is not None:
            raise NotImplementedError("RotatE runs on one GPU: the data-parallel exchange of the plain RotatE step is not built "
                                      "(launch it without torch.distributed, or with one rank)")
        self.embedding_range = (self.args.gamma + self.epsilon) / self.args.dim
        self._define_variables()
        self._define_embed_graph()

    def _check_args(self):
        """rotate.py:43-50, before any table is made."""
        check_args(self, dict(init='uniform', alignment_module='sharing', neg_sampling='uniform', optimizer='Adam',
                              eval_metric='inner'))
        assert self.args.gamma > 0.0, "RotatE: gamma must be > 0"

    def _define_variables(self):
        """rotate.py:52-59: three float64 variables, drawn in the reference's order."""
        a, n_ent, n_rel = self.args, self.kgs.entities_num, self.kgs.relations_num
        re = init_embeddings([n_ent, a.dim], 're_ent_embeds', a.init, a.ent_l2_norm)
        im = init_embeddings([n_ent, a.dim], 'im_ent_embeds', a.init, a.ent_l2_norm)
        rel = init_embeddings([n_rel, a.dim], 'rel_embeds', a.init, a.rel_l2_norm)
        dev = re.var.device
        self.ent_embeds = ComplexEntityTable(re.raw(), im.raw(), a.ent_l2_norm, dev)
        self.rel_embeds = PhaseTable(rel.raw(), a.rel_l2_norm, dev)

    @property
    def re_ent_embeds(self):
        return self.ent_embeds.parts()[0]

    @property
    def im_ent_embeds(self):
        return self.ent_embeds.parts()[1]

    def _define_embed_graph(self):
        """rotate.py:95-112: the negatives' half divided by neg_triple_num, one optimiser."""
        k = self.args.neg_triple_num
        self.triple_loss = dict(loss='rotate-logsigmoid', gamma=self.args.gamma, neg_loss_div=k)
        self._trainer = RotateTrainer(self.ent_embeds, self.rel_embeds, self.args, k, neg_loss_div=k)
        self.triple_optimizer = self._trainer.cfg

    def _lookup(self, ids):
        """l2n?(re)[ids] + l2n?(im)[ids], not normalised again (rotate.py:121-137), device fp32 [n, pad4(dim)]."""
        return self.ent_embeds.lookup(ids, sum_norm=False)

    def save(self):
        """rotate.py:139-144: sklearn-normalised re + im, the evaluated phases, no mapping matrix; fp32 payloads like every
        other model's files."""
        re, im = self.ent_embeds.parts()
        ent = re + im
        norms = np.sqrt((ent * ent).sum(1, keepdims=True))
        ent = ent / np.where(norms == 0, 1.0, norms)
        rd.save_embeddings(self.out_folder, self.kgs, ent.astype(np.float32), self.rel_embeds.eval().astype(np.float32), None,
                           mapping_mat=None)
