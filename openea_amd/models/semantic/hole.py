"""HolE (openea/models/semantic/hole.py:9-86): holographic embeddings.  A triple scores by the circular correlation of its
(normalised) entity rows against its relation row, normalised once more (hole.py:55-60):
    c[k] = sum_i h[i] t[(i + k) mod d],   score = -sigmoid(l2_normalize(r) . c),
and the margin loss compares a positive with the mean score of its k negatives (hole.py:78-84).  One Adagrad trains
ent_embeds and rel_embeds.

Layout: the ordinary tables of BasicModel; the step is oea_semantic_step (csrc/semantic_step.hip) -- the three d x d
correlation sums in LDS, the row gradients into the step engine's scratch, its apply phase for the optimiser.  Evaluation
and save() are BasicModel's."""
from ... import ops
from ..basic_model import BasicModel
from .semantic_trainer import SemanticTrainer, check_args, check_device_path


class HolE(BasicModel):

    def init(self):
        check_device_path(self)
        self._define_variables()
        self._define_embed_graph()
        self._check_args()

    def _check_args(self):
        """hole.py:28-36."""
        check_args(self, dict(init='xavier', alignment_module='sharing', neg_sampling='uniform', optimizer='Adagrad',
                              eval_metric='inner', loss_norm='L2', ent_l2_norm=True, rel_l2_norm=True))
        assert self.args.margin > 0.0, "HolE: margin must be > 0"

    def _define_embed_graph(self):
        """hole.py:62-86."""
        a = self.args
        self.triple_loss = "sum relu(margin - sigmoid(r . ccorr(h, t)) + mean_k sigmoid(r' . ccorr(h', t')))"
        cfg = ops.make_step_cfg(loss='margin-based', margin=a.margin, ent_l2_norm=self.ent_embeds.is_l2_norm,
                                rel_l2_norm=self.rel_embeds.is_l2_norm, optimizer=a.optimizer, lr=a.learning_rate,
                                neg_group_k=a.neg_triple_num)
        self.triple_optimizer = cfg
        self._trainer = SemanticTrainer(ops.SEMANTIC_HOLE, self.ent_embeds, self.rel_embeds, cfg, a.optimizer)
