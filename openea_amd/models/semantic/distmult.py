"""DistMult (openea/models/semantic/distmult.py:15-87): a triple scores by the trilinear product of its (normalised) rows,
    score(h, r, t) = sum_d h[d] r[d] t[d],
and the loss is the MEAN of softplus(-label * score) over the labelled batch -- the positives with label +1 followed by their
negatives with label -1 (distmult.py:56-58, batch.py:generate_triple_label_batch).  The loss does not depend on the order of
that list, so RelationTripleEpochs supplies (pos, neg) in the sampler's layout.

The reference ignores args.optimizer and always builds Adagrad (distmult.py:59).  Here any other args.optimizer is refused
rather than silently overridden.

Layout: the ordinary tables of BasicModel; the step is oea_semantic_step with OEA_SEMANTIC_DISTMULT (csrc/semantic_step.hip).
The epoch line is the reference's own: the sum of the batch means, undivided (distmult.py:87).  Evaluation and save() are
BasicModel's."""
import time

from ... import ops
from ..basic_model import BasicModel
from .semantic_trainer import SemanticTrainer, check_args, check_device_path


class DistMult(BasicModel):

    def __init__(self):
        super().__init__()
        self.metric = 'inner'

    def init(self):
        self._check_args()
        check_device_path(self)
        self._define_variables()
        self._define_embed_graph()

    def _check_args(self):
        check_args(self, dict(alignment_module='sharing', neg_sampling='uniform', optimizer='Adagrad'))

    def _define_embed_graph(self):
        """distmult.py:46-59."""
        a = self.args
        self.triple_loss = "mean softplus(-label * sum_d h r t)"
        cfg = ops.make_step_cfg(loss='margin-based', ent_l2_norm=self.ent_embeds.is_l2_norm,
                                rel_l2_norm=self.rel_embeds.is_l2_norm, optimizer=a.optimizer, lr=a.learning_rate,
                                neg_group_k=a.neg_triple_num)
        self.triple_optimizer = cfg
        self._trainer = SemanticTrainer(ops.SEMANTIC_DISTMULT, self.ent_embeds, self.rel_embeds, cfg, a.optimizer)

    def launch_triple_training_1epo(self, epoch, triple_steps, steps_tasks, batch_queue, neighbors1, neighbors2):
        """distmult.py:61-87: the epoch loss is the sum of the batch means."""
        start = time.time()
        self._ensure_epochs(True).run_epoch(self._trainer)
        epoch_loss = self._trainer.pop_loss()
        print('epoch {}, triple loss: {:.4f}, cost time: {:.4f}s'.format(epoch, epoch_loss, time.time() - start))
