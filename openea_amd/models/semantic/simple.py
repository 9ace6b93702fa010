"""SimplE (openea/models/semantic/simple.py:12-115): a head and a tail table per entity, two relation tables, and each
triple scored both ways (simple.py:62-88),
    score(h, r, t) = (l2_normalize(H[h] o R1[r]) . T[t] + l2_normalize(H[t] o R2[r]) . T[h]) / 2,
loss = sum_pos softplus(-score) + sum_neg softplus(score); the four tables are l2-normalised at lookup and one Adagrad trains
them all.

Layout: the four variables live in TWO device tables, as TransD's do -- rows [0, E) of `ent_embeds` are H and rows [E, 2E)
are T, rows [0, R) / [R, 2R) of `rel_embeds` are R1 / R2 -- so the step engine's scratch and apply phase serve them with
no second code path.  The step is oea_semantic_step (csrc/semantic_step.hip).  Evaluation embeddings are l2n(H) + l2n(T)
(simple.py:90-108), computed on the device."""
import numpy as np

from ... import ops
from ...modules.base.initializers import init_embeddings
from ...modules.load import read as rd
from ..basic_model import BasicModel
from ..trainer import EmbeddingTable
from .semantic_trainer import SemanticTrainer, check_args, check_device_path


def _stacked(first, second, name):
    return EmbeddingTable(np.concatenate([first.raw(), second.raw()]), first.is_l2_norm, name, dev=first.var.device,
                          visible_rows=first.rows)


class SimplE(BasicModel):

    def init(self):
        check_device_path(self)
        self._define_variables()
        self._define_embed_graph()
        self._check_args()

    def _check_args(self):
        """simple.py:28-34."""
        check_args(self, dict(init='xavier', alignment_module='sharing', neg_sampling='uniform', optimizer='Adagrad',
                              eval_metric='inner', ent_l2_norm=True, rel_l2_norm=True))

    def _define_variables(self):
        """simple.py:36-47: the four init_embeddings calls in the reference's order, then stacked pairwise."""
        a, n_ent, n_rel = self.args, self.kgs.entities_num, self.kgs.relations_num
        head = init_embeddings([n_ent, a.dim], 'head_ent_embeds', a.init, a.ent_l2_norm)
        tail = init_embeddings([n_ent, a.dim], 'tail_ent_embeds', a.init, a.ent_l2_norm)
        rel1 = init_embeddings([n_rel, a.dim], 'rel_embeds1', a.init, a.rel_l2_norm)
        rel2 = init_embeddings([n_rel, a.dim], 'rel_embeds2', a.init, a.rel_l2_norm)
        self.ent_embeds = _stacked(head, tail, 'ent_embeds')
        self.rel_embeds = _stacked(rel1, rel2, 'rel_embeds')

    def _define_embed_graph(self):
        """simple.py:62-88."""
        a = self.args
        self.triple_loss = "sum_pos softplus(-score) + sum_neg softplus(score)"
        cfg = ops.make_step_cfg(loss='margin-based', ent_l2_norm=self.ent_embeds.is_l2_norm,
                                rel_l2_norm=self.rel_embeds.is_l2_norm, optimizer=a.optimizer, lr=a.learning_rate,
                                neg_group_k=a.neg_triple_num)
        self.triple_optimizer = cfg
        self._trainer = SemanticTrainer(ops.SEMANTIC_SIMPLE, self.ent_embeds, self.rel_embeds, cfg, a.optimizer)

    def _lookup(self, ids):
        """l2n(H)[ids] + l2n(T)[ids] (simple.py:90-108), device [n, ld]."""
        e = self.ent_embeds
        if not hasattr(ids, "is_cuda"):
            ids = ops.to_ids(np.asarray(ids, np.int32), e.var.device)
        return e.lookup(ids) + e.lookup(ids + e.visible_rows)

    def _half(self, table, second):
        lo, hi = (table.visible_rows, table.rows) if second else (0, table.visible_rows)
        return table.lookup(np.arange(lo, hi, dtype=np.int32))[:, :table.dim].cpu().numpy()

    @property
    def head_ent_embeds(self):
        """host [E, dim]: l2n(H), as `self.head_ent_embeds.eval()` gave it."""
        return self._half(self.ent_embeds, False)

    @property
    def tail_ent_embeds(self):
        return self._half(self.ent_embeds, True)

    @property
    def rel_embeds1(self):
        return self._half(self.rel_embeds, False)

    @property
    def rel_embeds2(self):
        return self._half(self.rel_embeds, True)

    def save(self):
        """simple.py:110-115: ent = normalize(l2n(H) + l2n(T)) (sklearn row normalisation), rel = l2n(R1) + l2n(R2)."""
        d = self.args.dim
        ent = self._lookup(np.arange(self.ent_embeds.visible_rows, dtype=np.int32))
        ops.normalize_rows_(ent, d, sklearn=True)
        r = self.rel_embeds
        rel = r.lookup(np.arange(r.visible_rows, dtype=np.int32)) + r.lookup(np.arange(r.visible_rows, r.rows, dtype=np.int32))
        rd.save_embeddings(self.out_folder, self.kgs, ent[:, :d].cpu().numpy(), rel[:, :d].cpu().numpy(), None,
                           mapping_mat=None)
