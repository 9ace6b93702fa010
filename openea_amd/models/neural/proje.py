"""ProjE (openea/models/neural/proje.py:17-112): the head and the relation of a triple, each batch-normalised, are combined by
a diagonal layer, batch-normalised again and scored against every entity's output vector; training is a sampled softmax
(tf.nn.nce_loss) over dnn_neg_nums log-uniform candidates shared by the batch, under Adam:
    out = (BN(l2n(ent)[h]) + BN(l2n(rel)[r])) o mlp_w + mlp_bias,  x = BN'(out),
    loss = sum_b [xent(x_b . W[t_b] + b[t_b] - log Q(t_b), 1) + sum_j xent(x_b . W[s_j] + b[s_j] - log Q(s_j), 0)].
There are no negative triples.  Eight variables: ent_embeds, rel_embeds, entity_w, entity_b, the shared input beta, mlp_w,
mlp_bias and the output beta (batch_norm's moving averages are never read and are not kept).

The step is oea_proje_step (csrc/proje_step.hip): sampler, projection, the two MFMA sweeps of the NCE half and dense Adam.
Evaluation, save() and predict() are BasicModel's, on l2n(ent_embeds) under the inner product."""
import math
import time

import numpy as np

from ... import ops
from ...modules.base import initializers
from ...modules.base.initializers import init_embeddings
from ...modules.finding.evaluation import early_stop
from ...modules.utils.util import task_divide
from ..basic_model import BasicModel
from .proje_trainer import ProjETrainer, check_device_path


class ProjE(BasicModel):

    def __init__(self):
        super().__init__()
        self.entity_w = None
        self.entity_b = None

    def init(self):
        check_device_path(self)
        self._define_variables()
        self._define_embed_graph()
        self.check_args()

    def check_args(self):
        """proje.py:28-34."""
        a = self.args
        assert a.init == 'xavier'
        assert a.alignment_module == 'sharing'
        assert a.optimizer == 'Adam'
        assert a.eval_metric == 'inner'
        assert a.ent_l2_norm is True
        assert a.rel_l2_norm is True
        assert a.dnn_neg_nums > 1

    def _define_variables(self):
        """proje.py:36-44 (+ the variables its graph creates with get_variable / batch_norm, :54-62)."""
        a, E, R = self.args, self.kgs.entities_num, self.kgs.relations_num
        self.ent_embeds = init_embeddings([E, a.dim], 'ent_embeds', a.init, a.ent_l2_norm)
        self.rel_embeds = init_embeddings([R, a.dim], 'rel_embeds', a.init, a.rel_l2_norm)
        self.entity_w = init_embeddings([E, a.dim], 'entity_w', 'xavier', False)
        self.entity_b = init_embeddings([E, ], 'entity_b', 'xavier', False)
        dev = self.ent_embeds.var.device
        self.input_bn_beta = ops.to_vec(np.zeros(a.dim, np.float32), dev)
        self.mlp_w = ops.to_vec(initializers.glorot_uniform_host(initializers._rng, (a.dim,)), dev)
        self.mlp_bias = ops.to_vec(initializers.glorot_uniform_host(initializers._rng, (a.dim,)), dev)
        self.output_bn_beta = ops.to_vec(np.zeros(a.dim, np.float32), dev)

    def variables(self):
        """the eight trainable variables as device tensors, in the order of ops.PROJE_VARS"""
        return [self.ent_embeds.var, self.rel_embeds.var, self.entity_w.var, self.entity_b, self.input_bn_beta, self.mlp_w,
                self.mlp_bias, self.output_bn_beta]

    def _define_embed_graph(self):
        """proje.py:46-74."""
        a = self.args
        if not a.dnn_neg_nums > 1:
            raise AssertionError("ProjE: dnn_neg_nums must be > 1")
        n_sampled = min(int(a.dnn_neg_nums), self.kgs.entities_num)
        self.triple_loss = "sum nce_loss(weights=entity_w, biases=entity_b, labels=t, inputs=bn(mlp(bn(h), bn(r))), num_sampled)"
        self.triple_optimizer = dict(optimizer='Adam', learning_rate=a.learning_rate)
        b = self._ensure_epochs(False).batches
        self._trainer = ProjETrainer(self.variables(), a.dim, n_sampled, a.learning_rate, b.b1 + b.b2, seed=self._seed)

    def launch_triple_training_1epo(self, epoch, triple_steps, steps_tasks, batch_queue, neighbors1, neighbors2):
        """proje.py:76-96: positive batches only (made on the device), the printed loss is sum batch loss / sum |batch|."""
        start = time.time()
        trained_samples_num = self._ensure_epochs(False).run_epoch(self._trainer)
        epoch_loss = self._trainer.pop_loss() / max(trained_samples_num, 1)
        print('epoch {}, avg. triple loss: {:.4f}, cost time: {:.4f}s'.format(epoch, epoch_loss, time.time() - start))

    def run(self):
        """proje.py:98-112."""
        t = time.time()
        triples_num = self.kgs.kg1.relation_triples_num + self.kgs.kg2.relation_triples_num
        triple_steps = int(math.ceil(triples_num / self.args.batch_size))
        steps_tasks = task_divide(list(range(triple_steps)), self.args.batch_threads_num)
        for i in range(1, self.args.max_epoch + 1):
            self.launch_training_1epo(i, triple_steps, steps_tasks, None, None, None)
            if i >= self.args.start_valid and i % self.args.eval_freq == 0:
                flag = self.valid(self.args.stop_metric)
                self.flag1, self.flag2, self.early_stop = early_stop(self.flag1, self.flag2, flag)
                if self.early_stop or i == self.args.max_epoch:
                    break
        if self._epochs is not None:
            self._epochs.check()
        print("Training ends. Total time = {:.3f} s.".format(time.time() - t))
