"""ConvE (openea/models/neural/conve.py:21-79): ProjE's graph with a convolutional front end.  The normalised head and relation
rows are stacked into a [2x, y] image (x y = dim), batch-normalised, dropped out, convolved 3 x 3 ('same') into filter_num
channels, batch-normalised, rectified, dropped out, flattened to 2 dim filter_num values, sent through a dense relu layer back
to dim, batch-normalised, and scored with ProjE's sampled softmax (tf.nn.nce_loss) under Adam.  tf.layers.batch_normalization is
called without training=: it is the affine map v gamma / sqrt(1 + 1e-3) + beta on the initial moving statistics.  Fourteen
variables (ops.CONVE_VARS).

The step is oea_conve_step (csrc/conve_step.hip).  run(), the epoch loop, evaluation, save() and predict() are ProjE's /
BasicModel's."""
import math

import numpy as np

from ... import ops
from ...modules.base import initializers
from .conve_trainer import ConvETrainer, check_device_path
from .proje import ProjE


def dim_factorization(d):
    """conve.py:10-18"""
    x, y = ops.dim_factorization(d)
    assert x * y == d
    print("dim factorization", x, y)
    return x, y


def _uniform(shape, fan_in, fan_out):
    lim = math.sqrt(6.0 / (fan_in + fan_out))
    return initializers._rng.uniform(-lim, lim, tuple(shape)).astype(np.float32)


class ConvE(ProjE):

    def __init__(self):
        super().__init__()
        self.kernel_size = (3, 3)
        print("kernel_size", self.kernel_size)

    def init(self):
        check_device_path(self)
        self._define_variables()
        self._define_embed_graph()
        self.check_args()

    def _define_variables(self):
        """proje.py:36-44 for the four tables; the ten variables conve.py:53-64 creates through tf.layers / tf.contrib.layers:
        batch_normalization gamma ones / beta zeros, conv2d kernel [3, 3, 1, F] glorot-uniform (fans 9 and 9 F) with a zero bias,
        fully_connected weights xavier-uniform (fans 2 dim F and dim) with zero biases."""
        a, E, R = self.args, self.kgs.entities_num, self.kgs.relations_num
        F, d = int(a.filter_num), int(a.dim)
        y = ops.dim_factorization(d)[1]
        self.ent_embeds = initializers.init_embeddings([E, d], 'ent_embeds', a.init, a.ent_l2_norm)
        self.rel_embeds = initializers.init_embeddings([R, d], 'rel_embeds', a.init, a.rel_l2_norm)
        self.entity_w = initializers.init_embeddings([E, d], 'entity_w', 'xavier', False)
        self.entity_b = initializers.init_embeddings([E, ], 'entity_b', 'xavier', False)
        dev = self.ent_embeds.var.device
        ones, zeros = (lambda n: ops.to_vec(np.ones(n, np.float32), dev)), (lambda n: ops.to_vec(np.zeros(n, np.float32), dev))
        self.bn1_gamma, self.bn1_beta = ones(y), zeros(y)
        self.conv_kernel = ops.to_vec(_uniform((3, 3, 1, F), 9, 9 * F).reshape(-1), dev)
        self.conv_bias = zeros(F)
        self.bn2_gamma, self.bn2_beta = ones(F), zeros(F)
        self.fc_w = ops.to_table(_uniform((2 * d * F, d), 2 * d * F, d), dev=dev)
        self.fc_b = zeros(d)
        self.bn3_gamma, self.bn3_beta = ones(d), zeros(d)

    def variables(self):
        """the fourteen trainable variables as device tensors, in the order of ops.CONVE_VARS"""
        return [self.ent_embeds.var, self.rel_embeds.var, self.entity_w.var, self.entity_b, self.bn1_gamma, self.bn1_beta,
                self.conv_kernel, self.conv_bias, self.bn2_gamma, self.bn2_beta, self.fc_w, self.fc_b, self.bn3_gamma, self.bn3_beta]

    def _define_embed_graph(self):
        """conve.py:42-79."""
        a = self.args
        if not a.dnn_neg_nums > 1:
            raise AssertionError("ConvE: dnn_neg_nums must be > 1")
        dim_factorization(a.dim)
        n_sampled = min(int(a.dnn_neg_nums), self.kgs.entities_num)
        self.triple_loss = "sum nce_loss(weights=entity_w, biases=entity_b, labels=t, inputs=bn(fc(drop(relu(bn(conv(drop(bn([h; r])))))))))"
        self.triple_optimizer = dict(optimizer='Adam', learning_rate=a.learning_rate)
        b = self._ensure_epochs(False).batches
        self._trainer = ConvETrainer(self.variables(), a.dim, a.filter_num, a.output_keep_prob, n_sampled, a.learning_rate,
                                     b.b1 + b.b2, seed=self._seed)
