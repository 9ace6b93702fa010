"""TransR (openea/models/trans/transr.py:9-50): every relation has a d x d matrix; both entities of a triple are projected
with their triple's relation matrix and normalised before the translation,
    h' = l2_normalize(M_r l2_normalize(ent)[h]),   t' likewise,   r = l2_normalize(rel)[r] (not projected),
and TransE's margin loss is taken on the projected rows (transr.py:33-50).  One optimiser covers the three variables.

Layout: `ent_embeds` / `rel_embeds` are the ordinary tables of the fused step; `rel_matrix` is a plain device fp32 tensor
[R, d*d] (row-major d x d per relation, not normalised) with its own Adagrad accumulator.  The step is oea_transr_step
(csrc/transr_step.hip): projections grouped by relation on the fp32 matrix cores, the matrix update inside the call, the
entity / relation rows finished by the step engine's apply phase.  Evaluation and save() see ent_embeds / rel_embeds only,
as in the reference (basic_model.py:184-188)."""
import torch

from ... import ops
from ...modules.base.initializers import init_embeddings
from ...modules.base.losses import get_loss_func
from ...modules.base.optimizers import generate_optimizer
from .transe import TransE


class TransRTrainer:
    """One optimiser instance over ent_embeds, rel_embeds and rel_matrix (generate_optimizer, transr.py:49-50).  Same interface
    as TripleTrainer (step / pop_loss / dist) without the fused epoch call: RelationTripleEpochs drives it step by step."""
    fused_epoch = False

    def __init__(self, ent, rel, rel_matrix, cfg, optimizer):
        if optimizer not in ('Adagrad', 'SGD'):
            raise NotImplementedError("TransR: optimizer=%s -- the TransR step trains with Adagrad (the shipped args file) or SGD"
                                      % optimizer)
        self.ent, self.rel, self.rel_matrix, self.cfg = ent, rel, rel_matrix, cfg
        dev = ent.var.device
        if optimizer == 'Adagrad':        # tf.train.AdagradOptimizer: initial_accumulator_value = 0.1
            self.ent_acc = torch.full_like(ent.var, 0.1)
            self.rel_acc = torch.full_like(rel.var, 0.1)
            self.rel_matrix_acc = torch.full_like(rel_matrix, 0.1)
        else:
            self.ent_acc = self.rel_acc = self.rel_matrix_acc = None
        self.ws = ops.step_workspace(ent.rows, rel.rows, ent.ld, dev)
        self.loss = torch.zeros(1, dtype=torch.float64, device=dev)
        self.dist = None
        self.t = 0
        self._tr_ws, self._tr_cap = None, -1

    def step(self, pos, neg):
        """pos / neg: device int32 [n, 3], neg i the corruption of pos i."""
        n = pos.shape[0]
        if n > self._tr_cap:
            self._tr_ws = ops.transr_workspace(self.ent.rows, self.rel.rows, self.ent.dim, n, self.ent.var.device)
            self._tr_cap = n
        self.t += 1
        ops.transr_step(self.ent.var, self.ent_acc, self.rel.var, self.rel_acc, self.rel_matrix, self.rel_matrix_acc,
                        self.ent.dim, pos, neg, self.cfg, self.ws, self._tr_ws, self.loss)

    def pop_loss(self):
        v = float(self.loss.item())
        self.loss.zero_()
        return v


class TransR(TransE):

    def init(self):
        if self._dist_group() is not None:
            raise NotImplementedError("TransR runs on one GPU: the data-parallel exchange of the relation-matrix gradients is "
                                      "not built (launch it without torch.distributed, or with one rank)")
        if self.args.dim > ops.TRANSR_MAX_DIM:
            raise NotImplementedError("TransR: dim %d > %d (the TransR step stages a whole relation matrix in LDS)"
                                      % (self.args.dim, ops.TRANSR_MAX_DIM))
        super().init()

    def _define_variables(self):
        """transr.py:14-21: the three init_embeddings calls in the reference's order; rel_matrix is not normalised."""
        a, n_ent, n_rel = self.args, self.kgs.entities_num, self.kgs.relations_num
        self.ent_embeds = init_embeddings([n_ent, a.dim], 'ent_embeds', a.init, a.ent_l2_norm)
        self.rel_embeds = init_embeddings([n_rel, a.dim], 'rel_embeds', a.init, a.rel_l2_norm)
        m = init_embeddings([n_rel, a.dim * a.dim], 'rel_matrix', a.init, False)
        self._rel_matrix = m.var[:, :a.dim * a.dim].contiguous()
        del m

    @property
    def rel_matrix(self):
        """host [R, d*d], as `self.rel_matrix.eval()` gave it."""
        return self._rel_matrix.cpu().numpy()

    def _define_embed_graph(self):
        """transr.py:23-50."""
        self.triple_loss = get_loss_func(self.args)
        merged = generate_optimizer(self.triple_loss, self.args.learning_rate, opt=self.args.optimizer)
        cfg = ops.make_step_cfg(ent_l2_norm=self.ent_embeds.is_l2_norm, rel_l2_norm=self.rel_embeds.is_l2_norm,
                                neg_group_k=0, **merged)
        self.triple_optimizer = cfg
        self._trainer = TransRTrainer(self.ent_embeds, self.rel_embeds, self._rel_matrix, cfg, merged['optimizer'])
