"""Golden loss and gradients of ConvE's graph, from the REFERENCE's own code (models/neural/conve.py: ProjE._define_variables and
ConvE._define_embed_graph run unmodified under tests/golden/tf_shim.py through the helpers of make_tf_graph_golden.py and
make_proje_golden.py).  The stand-in lacks what this file uses; it is supplied here, on the stand-in module, without editing it:
  layers.batch_normalization        inference mode on the initial moving statistics: x gamma / sqrt(1 + 1e-3) + beta along `axis`
  layers.conv2d                     'same', channels_first, kernel [3, 3, 1, F] glorot-uniform, zero bias, cross-correlation
  contrib.layers.fully_connected    relu(x W + b), W xavier-uniform, zero biases
  nn.dropout                        v / keep_prob * mask; the masks are the numpy restatement of the project's Philox definition
                                    (tests/test_conve_cpu.py: mask_lanes), layer = the order of the calls, and are recorded
  nn.nce_loss, variable_scope       as in make_proje_golden.py
These are TF-1's documented semantics, stated as assumptions A1-A10 in tests/test_proje_cpu.py and tests/test_conve_cpu.py; no
fixture pins them.  Cases:
  'conve_d6'   E = 14, R = 4, d = 6 (a 6 x 2 image),  F = 3, B = 6,  S = 4
  'conve_d16'  E = 40, R = 5, d = 16 (an 8 x 4 image), F = 3, B = 10, S = 12
Each batch holds a repeated head, a repeated label, a label that is among the samples and one triple with h == t.  The loss is
evaluated in float64 at float32-representable variable values; the gradients w.r.t. all fourteen variables are central finite
differences.  No relu pre-activation lies within 1e-4 of zero (asserted), so no difference straddles a kink.  Arrays only.

Run in the build container only:  python tests/golden/make_conve_golden.py   -> tests/golden/conve_graph.npz
"""
import importlib
import os
import sys
import types

import numpy as np

from make_tf_graph_golden import HERE, REPO, fd_gradients, import_reference, quiet
from make_proje_golden import SEED, _FEED, _batch, _extend_standin

sys.path.insert(0, os.path.join(REPO, 'tests'))
from test_conve_cpu import VARS, mask_lanes, mask_threshold  # noqa: E402
from test_proje_cpu import log_uniform_reference  # noqa: E402

MASK_STEP = 3
KEEP = 0.7
VAR_SEED = 31


def _extend_for_conve(tf, record):
    shim = sys.modules['tensorflow']

    def width(x, axis):
        return np.shape(tf.evaluate(x, _FEED[0]))[axis]

    def batch_normalization(inputs, axis=-1, **_):
        n = width(inputs, axis)
        k = len(record['bn']) + 1
        gamma, beta = tf.Variable(np.ones(n), name='bn%d/gamma' % k), tf.Variable(np.zeros(n), name='bn%d/beta' % k)
        record['bn'].append((gamma, beta))

        def fn(x, g, b):
            shape = [1] * x.ndim
            shape[axis] = -1
            return x * (g.reshape(shape) / np.sqrt(1.0 + 1e-3)) + b.reshape(shape)
        return tf.Node(fn, inputs, gamma, beta)

    def conv2d(inputs, filters, kernel_size, padding='valid', use_bias=True, data_format='channels_last', **_):
        assert padding == 'same' and data_format == 'channels_first' and use_bias and tuple(kernel_size) == (3, 3)
        assert width(inputs, 1) == 1
        lim = np.sqrt(6.0 / (9 + 9 * filters))
        kernel = tf.Variable(tf._RNG.uniform(-lim, lim, (3, 3, 1, filters)), name='cnn/conv2d/kernel')
        bias = tf.Variable(np.zeros(filters), name='cnn/conv2d/bias')

        def fn(x, k, b):
            n, _, rows, cols = x.shape
            xp = np.pad(x[:, 0], ((0, 0), (1, 1), (1, 1)))
            out = np.zeros((n, filters, rows, cols))
            for i in range(rows):
                for j in range(cols):
                    out[:, :, i, j] = np.einsum('nab,abf->nf', xp[:, i:i + 3, j:j + 3], k[:, :, 0, :])
            return out + b[None, :, None, None]
        return tf.Node(fn, inputs, kernel, bias)

    def relu(x):
        def fn(v):
            if record['watch']:
                record['min_pre'] = min(record['min_pre'], float(np.abs(v).min()))
            return np.maximum(v, 0.0)
        return tf.Node(fn, x)

    def fully_connected(inputs, num_outputs, **_):
        n_in = width(inputs, -1)
        lim = np.sqrt(6.0 / (n_in + num_outputs))
        weights = tf.Variable(tf._RNG.uniform(-lim, lim, (n_in, num_outputs)), name='fully_connected/weights')
        biases = tf.Variable(np.zeros(num_outputs), name='fully_connected/biases')
        return relu(tf.Node(lambda x, w, b: x @ w + b, inputs, weights, biases))

    def dropout(x, keep_prob=None, **_):
        layer = record['n_dropout']
        record['n_dropout'] += 1
        assert keep_prob == KEEP and layer < 2

        def fn(v):
            n = int(np.prod(v.shape[1:]))
            m = np.stack([mask_lanes(SEED, MASK_STEP, layer, b, n) < mask_threshold(keep_prob) for b in range(v.shape[0])])
            if record['watch']:
                record['m%d' % layer] = m.astype(np.float64)
            return v / keep_prob * m.reshape(v.shape)
        return tf.Node(fn, x)

    shim.layers.batch_normalization = batch_normalization
    shim.layers.conv2d = conv2d
    shim.contrib.layers.fully_connected = fully_connected
    shim.nn.relu = relu
    shim.nn.dropout = dropout


def main():
    ref = import_reference()
    tf = ref.tf
    record = {}
    registry = _extend_standin(tf, record)
    _extend_for_conve(tf, record)
    ConvE = importlib.import_module('openea.models.neural.conve').ConvE
    from openea_amd.run.default_args import get_args
    rng = np.random.RandomState(VAR_SEED)
    out = {}
    for tag, n_ent, n_rel, d, n_s, F in (('conve_d6', 14, 4, 6, 4, 3), ('conve_d16', 40, 5, 16, 12, 3)):
        del tf.VARIABLES[:]
        registry.clear()
        record.update(bn=[], n_dropout=0, watch=False, min_pre=np.inf)
        sampled, num_tries, _ = log_uniform_reference(n_ent, n_s, SEED, 0)
        pos = _batch('proje_d5' if tag == 'conve_d6' else 'proje_d16', sampled)
        assert pos[:, 2].max() < n_ent and (pos[:, 0] == pos[:, 2]).sum() == 1 and set(pos[:, 2]) & set(sampled)
        m = quiet(ConvE)
        quiet(m.set_args, get_args('ConvE', dim=d, dnn_neg_nums=n_s, filter_num=F, output_keep_prob=KEEP, output='/tmp/oea_golden/',
                                   training_data='synthetic/tiny/', dataset_division='f/'))
        m.set_kgs(types.SimpleNamespace(entities_num=n_ent, relations_num=n_rel))
        m._define_variables()
        _FEED[0] = {}
        orig_placeholder = sys.modules['tensorflow'].placeholder

        def placeholder(dtype=None, shape=None, name=None):
            p = orig_placeholder(dtype, shape, name)
            _FEED[0][p] = np.zeros(2, np.int64)
            return p
        sys.modules['tensorflow'].placeholder = placeholder
        quiet(m._define_embed_graph)
        sys.modules['tensorflow'].placeholder = orig_placeholder
        variables = list(tf.VARIABLES)
        assert len(variables) == 14, [v.name for v in variables]
        shapes = [v.data.shape for v in variables]
        assert shapes[4] == shapes[5] and shapes[6] == (3, 3, 1, F) and shapes[7] == shapes[8] == shapes[9] == (F,), shapes
        assert shapes[10] == (2 * d * F, d) and shapes[11] == shapes[12] == shapes[13] == (d,), shapes
        assert np.array_equal(record['sampled'], sampled) and record['num_tries'] == num_tries
        for v in variables:                      # float32-representable values, moderately sized
            v.data = (rng.standard_normal(v.data.shape) * 0.6).astype(np.float32).astype(np.float64)
        feed = {m.pos_hs: pos[:, 0], m.pos_rs: pos[:, 1], m.pos_ts: pos[:, 2]}
        record['watch'] = True
        value = float(tf.evaluate(m.triple_loss, feed))
        record['watch'] = False
        assert record['min_pre'] > 1e-4, (tag, record['min_pre'])
        grads = fd_gradients(tf, m.triple_loss, feed, variables)
        out[tag + '_pos'] = pos
        out[tag + '_sampled'] = np.asarray(sampled, np.int64)
        out[tag + '_num_tries'] = np.array([num_tries], np.int64)
        out[tag + '_shape'] = np.array([n_ent, n_rel, d, n_s, F, SEED, MASK_STEP])
        out[tag + '_keep_prob'] = np.array([KEEP])
        out[tag + '_m0'], out[tag + '_m1'] = record['m0'], record['m1']
        out[tag + '_loss'] = np.array([value])
        for name, v, g in zip(VARS, variables, grads):
            out['%s_var_%s' % (tag, name)] = v.data.copy()
            out['%s_grad_%s' % (tag, name)] = g
        print('%-10s loss %.6f  sampled %s  num_tries %d  min |relu pre-activation| %.3g  image %s'
              % (tag, value, list(sampled), num_tries, record['min_pre'], shapes[4]))
    np.savez_compressed(os.path.join(HERE, 'conve_graph.npz'), **out)


if __name__ == '__main__':
    main()
