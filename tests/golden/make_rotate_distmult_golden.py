"""Golden loss and gradients of RotatE's and DistMult's graphs, from the REFERENCE's own code (models/semantic/rotate.py and
distmult.py, run unmodified under tests/golden/tf_shim.py through the helpers of make_tf_graph_golden.py).  The one op the
stand-in lacks for these two files -- nn.softplus (DistMult's loss) -- is supplied here, on the stand-in module, without
editing it; cos / sin / sigmoid / log and the `dtype` argument of the initialisers are the stand-in's own.  Cases, each one
batch:
  'rotate_d6_k2'    E = 14, R = 4, d = 6,  k = 2   (gamma 3.0; the negatives' half of the loss divided by k, rotate.py:81)
  'rotate_d16_k3'   E = 24, R = 5, d = 16, k = 3
  'distmult_d5_k1'  E = 14, R = 4, d = 5,  k = 1
  'distmult_d16_k3' E = 24, R = 5, d = 16, k = 3
Every batch repeats entities, holds one triple with h == t and one negative whose relation differs from its positive's;
neg[p*k:(p+1)*k] are the negatives of positive p.  DistMult is fed the labelled list as generate_triple_label_batch builds it
(batch.py:168-183): the positives, then the negatives, labels +1 / -1.

The loss is evaluated in float64 at float32-representable variable values.  Its gradient w.r.t. every variable is taken by
central differences at two step sizes, h and 2 h, and extrapolated, g = (4 g_h - g_2h) / 3, which removes the h^2 term of
the truncation error.  The step-size check repeats that with (2 h, 4 h): the largest difference of the two extrapolations,
relative to the largest gradient entry, is printed and stored as '<case>_fd_err' -- it bounds what is left of truncation and
rounding together, and it is the figure the fp64 device test of RotatE takes its tolerance from.

Run in the build container only:  python tests/golden/make_rotate_distmult_golden.py   -> tests/golden/rotate_distmult_graph.npz
"""
import importlib
import os
import sys
import types

import numpy as np

from make_tf_graph_golden import HERE, ROOT, fd_gradients, import_reference, quiet
from make_semantic_golden import D5_POS, D16_POS

FD_H = 2e-4
# Standard deviation of the variables' values.  The device test reads DistMult's gradient from the difference of an fp32 table
# across one SGD step of lr = 0.01, so an entry v resolves it to half an ulp of v over lr, 2^-24 |v| / 0.01.  The loss is a mean
# over N = n_pos (k + 1) triples and the rows are normalised, so the largest gradient entry is about 0.5 / N / |row| * 0.1: at
# N = 40 and 0.6 that is 6e-3, and an entry of 2 resolves it to 2e-3 of it only -- coarser than the 1e-3 the test asks.  Both
# scale in favour of small values (ulp with |v|, gradient with 1 / |row|): at 0.15 the resolution is 16 times finer.  RotatE's
# tables are fp64 on the device and keep the 0.6 of the other fixtures.
SCALE = {'RotatE': 0.6, 'DistMult': 0.15}


def _negatives(pos, k, rng, n_ent, n_rel):
    """k corruptions per positive, neg[p*k:(p+1)*k] (head or tail replaced); one of pair 3's with another relation"""
    neg = np.repeat(pos, k, axis=0)
    for i in range(len(neg)):
        neg[i, 0 if i % 2 else 2] = rng.randint(0, n_ent)
    neg[3 * k + k - 1, 1] = (pos[3, 1] + 1) % n_rel
    return neg


def _extend_standin(tf):
    """what rotate.py / distmult.py use and tf_shim.py does not have, on the `tensorflow` module the reference imports"""
    shim = sys.modules['tensorflow']
    shim.nn.softplus = lambda x, name=None: tf.Node(lambda v: np.logaddexp(0.0, v), x)
    m = types.ModuleType('openea.models.semantic')
    m.__path__ = [ROOT + '/models/semantic']
    sys.modules['openea.models.semantic'] = m


def _extrapolated(tf, loss, feed, variables, h):
    g1 = fd_gradients(tf, loss, feed, variables, eps=h)
    g2 = fd_gradients(tf, loss, feed, variables, eps=2 * h)
    return [(4.0 * a - b) / 3.0 for a, b in zip(g1, g2)]


def main():
    ref = import_reference()
    tf = ref.tf
    _extend_standin(tf)
    RotatE = importlib.import_module('openea.models.semantic.rotate').RotatE
    DistMult = importlib.import_module('openea.models.semantic.distmult').DistMult
    from openea_amd.run.default_args import get_args
    rng = np.random.RandomState(31)
    names = {'RotatE': ['re_ent_embeds', 'im_ent_embeds', 'rel_embeds'], 'DistMult': ['ent_embeds', 'rel_embeds']}
    out = {}
    for tag, cls, n_ent, n_rel, d, k, pos in (('rotate_d6_k2', RotatE, 14, 4, 6, 2, D5_POS),
                                              ('rotate_d16_k3', RotatE, 24, 5, 16, 3, D16_POS),
                                              ('distmult_d5_k1', DistMult, 14, 4, 5, 1, D5_POS),
                                              ('distmult_d16_k3', DistMult, 24, 5, 16, 3, D16_POS)):
        del tf.VARIABLES[:]
        name = cls.__name__
        neg = _negatives(pos, k, rng, n_ent, n_rel)
        extra = dict(gamma=3.0) if name == 'RotatE' else {}
        m = cls()
        quiet(m.set_args, get_args(name, dim=d, neg_triple_num=k, output='/tmp/oea_golden/', training_data='synthetic/tiny/',
                                   dataset_division='f/', **extra))
        m.set_kgs(types.SimpleNamespace(entities_num=n_ent, relations_num=n_rel))
        if name == 'RotatE':
            m.embedding_range = (m.args.gamma + m.epsilon) / m.args.dim          # rotate.py:37, the first line of init()
        m._define_variables()
        m._define_embed_graph()
        variables = list(tf.VARIABLES)
        assert [v.name for v in variables] == names[name], [v.name for v in variables]
        for v in variables:                      # float32-representable values, moderately sized
            v.data = (rng.standard_normal(v.data.shape) * SCALE[name]).astype(np.float32).astype(np.float64)
        if name == 'RotatE':
            feed = {m.pos_hs: pos[:, 0], m.pos_rs: pos[:, 1], m.pos_ts: pos[:, 2],
                    m.neg_hs: neg[:, 0], m.neg_rs: neg[:, 1], m.neg_ts: neg[:, 2]}
            out[tag + '_gamma'] = np.array([float(m.args.gamma)])
            out[tag + '_phase_scale'] = np.array([m.pi / m.embedding_range])
        else:
            batch = np.concatenate([pos, neg])
            label = np.concatenate([np.ones(len(pos)), -np.ones(len(neg))])
            feed = {m.hs: batch[:, 0], m.rs: batch[:, 1], m.ts: batch[:, 2], m.label: label}
        value = float(tf.evaluate(m.triple_loss, feed))
        grads = _extrapolated(tf, m.triple_loss, feed, variables, FD_H)
        check = _extrapolated(tf, m.triple_loss, feed, variables, 2 * FD_H)
        gmax = max(np.abs(g).max() for g in grads)
        fd_err = max(np.abs(a - b).max() for a, b in zip(grads, check)) / gmax
        out[tag + '_pos'], out[tag + '_neg'] = pos, neg
        out[tag + '_shape'] = np.array([n_ent, n_rel, d, k])
        out[tag + '_loss'] = np.array([value])
        out[tag + '_fd_err'] = np.array([fd_err])
        for v, g in zip(variables, grads):
            out['%s_var_%s' % (tag, v.name)] = v.data.copy()
            out['%s_grad_%s' % (tag, v.name)] = g
        print('%-16s loss %.6f  step-size check %.2e of the largest gradient entry (%.3g)  variables %s'
              % (tag, value, fd_err, gmax, [v.name for v in variables]))
    np.savez_compressed(os.path.join(HERE, 'rotate_distmult_graph.npz'), **out)


if __name__ == '__main__':
    main()
