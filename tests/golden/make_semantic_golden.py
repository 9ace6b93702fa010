"""Golden loss and gradients of HolE's and SimplE's graphs, from the REFERENCE's own code (models/semantic/hole.py and
simple.py, run unmodified under tests/golden/tf_shim.py through the helpers of make_tf_graph_golden.py).  The stand-in
lacks a few ops these two files use -- fft / ifft / conj / real / complex64 (HolE's circular correlation) and nn.softplus
(SimplE's loss) -- which are supplied here, on the stand-in module, without editing it; complex64 is evaluated as
complex128 so that the fixture stays float64.  Cases, each one batch:
  'hole_d5'    E = 14, R = 4, d = 5,  k = 1
  'hole_d16'   E = 24, R = 5, d = 16, k = 1
  'hole_k3'    E = 24, R = 5, d = 16, k = 3 (the positive against the mean of its three negatives, neg[p*k:(p+1)*k])
  'simple_d5'  E = 14, R = 4, d = 5,  k = 1
  'simple_d16' E = 24, R = 5, d = 16, k = 1
Every batch repeats entities, holds one triple with h == t and one negative whose relation differs from its positive's.
The loss is evaluated in float64 at float32-representable variable values and its gradient w.r.t. every variable is taken
by central finite differences.

Run in the build container only:  python tests/golden/make_semantic_golden.py   -> tests/golden/semantic_graph.npz
"""
import importlib
import os
import sys
import types

import numpy as np

from make_tf_graph_golden import HERE, ROOT, fd_gradients, import_reference, quiet

D5_POS = np.array([[0, 1, 2], [3, 1, 4], [0, 0, 6], [7, 2, 0], [8, 3, 9], [5, 2, 5]], np.int64)
D5_NEG = np.array([[0, 1, 10], [11, 1, 4], [12, 0, 6], [7, 3, 5], [8, 3, 13], [5, 2, 1]], np.int64)   # pair 3: relation 3, not 2
D16_POS = np.array([[0, 1, 2], [3, 1, 4], [0, 1, 6], [7, 2, 0], [8, 3, 9], [2, 1, 3], [10, 4, 11], [12, 1, 0],
                    [5, 0, 5], [13, 1, 14]], np.int64)
D16_NEG = np.array([[0, 1, 20], [21, 1, 4], [0, 1, 7], [7, 3, 1], [8, 3, 22], [2, 1, 23], [10, 4, 0], [12, 1, 15],
                    [16, 0, 5], [13, 1, 3]], np.int64)           # pair 3: the negative's relation (3) is not its positive's (2)


def _k3_negatives(pos, rng, n_ent):
    """three corruptions per positive, neg[p*3:(p+1)*3] (head or tail replaced); one of pair 3's with another relation"""
    neg = np.repeat(pos, 3, axis=0)
    for i in range(len(neg)):
        neg[i, 0 if i % 2 else 2] = rng.randint(0, n_ent)
    neg[3 * 3 + 1, 1] = (pos[3, 1] + 1) % 5
    return neg


def _extend_standin(tf):
    """the ops of hole.py / simple.py that tf_shim.py does not have, on the `tensorflow` module the reference imports"""
    shim = sys.modules['tensorflow']
    complex64 = np.complex64
    base_cast = shim.cast

    def cast(x, dtype=None, name=None):
        if dtype is complex64:
            return tf.Node(lambda v: np.asarray(v, np.complex128), x)
        return base_cast(x, dtype, name)
    unary = (lambda fn: (lambda x, name=None: tf.Node(fn, x)))
    shim.complex64 = complex64
    shim.cast = cast
    shim.fft = unary(lambda v: np.fft.fft(v, axis=-1))
    shim.ifft = unary(lambda v: np.fft.ifft(v, axis=-1))
    shim.conj = unary(np.conj)
    shim.real = unary(np.real)
    shim.nn.softplus = unary(lambda v: np.logaddexp(0.0, v))
    m = types.ModuleType('openea.models.semantic')
    m.__path__ = [ROOT + '/models/semantic']
    sys.modules['openea.models.semantic'] = m


def main():
    ref = import_reference()
    tf = ref.tf
    _extend_standin(tf)
    HolE = importlib.import_module('openea.models.semantic.hole').HolE
    SimplE = importlib.import_module('openea.models.semantic.simple').SimplE
    from openea_amd.run.default_args import get_args
    rng = np.random.RandomState(29)
    k3_neg = _k3_negatives(D16_POS, rng, 24)
    names = {'HolE': ['ent_embeds', 'rel_embeds'],
             'SimplE': ['head_ent_embeds', 'tail_ent_embeds', 'rel_embeds1', 'rel_embeds2']}
    out = {}
    for tag, cls, n_ent, n_rel, d, k, pos, neg in (('hole_d5', HolE, 14, 4, 5, 1, D5_POS, D5_NEG),
                                                   ('hole_d16', HolE, 24, 5, 16, 1, D16_POS, D16_NEG),
                                                   ('hole_k3', HolE, 24, 5, 16, 3, D16_POS, k3_neg),
                                                   ('simple_d5', SimplE, 14, 4, 5, 1, D5_POS, D5_NEG),
                                                   ('simple_d16', SimplE, 24, 5, 16, 1, D16_POS, D16_NEG)):
        del tf.VARIABLES[:]
        name = cls.__name__
        m = cls()
        quiet(m.set_args, get_args(name, dim=d, neg_triple_num=k, output='/tmp/oea_golden/', training_data='synthetic/tiny/',
                                   dataset_division='f/'))
        m.set_kgs(types.SimpleNamespace(entities_num=n_ent, relations_num=n_rel))
        m._define_variables()
        m._define_embed_graph()
        variables = list(tf.VARIABLES)
        assert [v.name for v in variables] == names[name], [v.name for v in variables]
        for v in variables:                      # float32-representable values, moderately sized
            v.data = (rng.standard_normal(v.data.shape) * 0.6).astype(np.float32).astype(np.float64)
        feed = {m.pos_hs: pos[:, 0], m.pos_rs: pos[:, 1], m.pos_ts: pos[:, 2],
                m.neg_hs: neg[:, 0], m.neg_rs: neg[:, 1], m.neg_ts: neg[:, 2]}
        value = float(np.real(tf.evaluate(m.triple_loss, feed)))
        grads = fd_gradients(tf, m.triple_loss, feed, variables)
        out[tag + '_pos'], out[tag + '_neg'] = pos, neg
        out[tag + '_shape'] = np.array([n_ent, n_rel, d, k])
        out[tag + '_margin'] = np.array([float(getattr(m.args, 'margin', 0.0))])
        out[tag + '_loss'] = np.array([value])
        for v, g in zip(variables, grads):
            out['%s_var_%s' % (tag, v.name)] = v.data.copy()
            out['%s_grad_%s' % (tag, v.name)] = np.real(g)
        print('%-10s loss %.6f  variables %s' % (tag, value, [v.name for v in variables]))
    np.savez_compressed(os.path.join(HERE, 'semantic_graph.npz'), **out)


if __name__ == '__main__':
    main()
