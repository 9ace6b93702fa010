"""Golden loss and gradients of SEA's mapping graph, from the REFERENCE's own code (approaches/sea.py, `_define_variables` and
`_define_embed_graph` run unmodified under tests/golden/tf_shim.py through the helpers of make_tf_graph_golden.py; the stand-in
needs no further ops).  Cases, each one batch of labelled links (a[i], b[i]) and unlabelled links (c[j], d[j]):
  'sea_d5'      E = 14, R = 4, d = 5,  n_l = 4, n_u = 5
  'sea_d16'     E = 24, R = 5, d = 16, n_l = 7, n_u = 4
  'sea_d5_nu0'  E = 14, R = 4, d = 5,  n_l = 4, n_u = 0 (the supervised half alone)
The first two repeat an entity inside the labelled block and share an entity between the labelled and the unlabelled block.
`mapping_loss` is evaluated in float64 at float32-representable variable values and its gradient w.r.t. every variable
(ent_embeds, rel_embeds, mapping_matrix_1, mapping_matrix_2) is taken by central finite differences.  The reference normalises the
mapped blocks with tf.nn.l2_normalize WITHOUT an axis (sea.py:84-92): the fixture holds what that computes.

Run in the build container only:  python tests/golden/make_sea_golden.py   -> tests/golden/sea_graph.npz
"""
import importlib
import os
import types

import numpy as np

from make_tf_graph_golden import HERE, fd_gradients, import_reference, quiet

CASES = (
    # tag, E, R, d, labelled (a, b), unlabelled (c, d)
    ('sea_d5', 14, 4, 5, ([0, 1, 0, 2], [7, 8, 9, 8]), ([3, 0, 4, 5, 6], [10, 11, 12, 13, 7])),
    ('sea_d16', 24, 5, 16, ([0, 1, 2, 1, 3, 4, 5], [12, 13, 14, 15, 16, 12, 17]), ([6, 7, 1, 8], [18, 19, 20, 13])),
    ('sea_d5_nu0', 14, 4, 5, ([0, 1, 0, 2], [7, 8, 9, 8]), ([], [])),
)
NAMES = ['ent_embeds', 'rel_embeds', 'mapping_matrix_1', 'mapping_matrix_2']


def main():
    ref = import_reference()
    tf = ref.tf
    SEA = importlib.import_module('openea.approaches.sea').SEA
    from openea_amd.run.default_args import get_args
    rng = np.random.RandomState(31)
    out = {}
    for tag, n_ent, n_rel, d, lab, unl in CASES:
        del tf.VARIABLES[:]
        m = SEA()
        quiet(m.set_args, get_args('SEA', dim=d, output='/tmp/oea_golden/', training_data='synthetic/tiny/', dataset_division='f/'))
        m.set_kgs(types.SimpleNamespace(entities_num=n_ent, relations_num=n_rel))
        m._define_variables()
        m._define_embed_graph()
        variables = list(tf.VARIABLES)
        assert [v.name for v in variables] == NAMES, [v.name for v in variables]
        for v in variables:                      # float32-representable values, moderately sized
            v.data = (rng.standard_normal(v.data.shape) * 0.6).astype(np.float32).astype(np.float64)
        ids = [np.asarray(x, np.int64) for x in (lab[0], lab[1], unl[0], unl[1])]
        feed = {m.labeled_entities1: ids[0], m.labeled_entities2: ids[1],
                m.unlabeled_entities1: ids[2], m.unlabeled_entities2: ids[3]}
        value = float(tf.evaluate(m.mapping_loss, feed))
        grads = fd_gradients(tf, m.mapping_loss, feed, variables)
        for key, x in zip(('l1', 'l2', 'u1', 'u2'), ids):
            out['%s_%s' % (tag, key)] = x
        out[tag + '_shape'] = np.array([n_ent, n_rel, d])
        out[tag + '_alpha'] = np.array([float(m.args.alpha_1), float(m.args.alpha_2)])
        out[tag + '_loss'] = np.array([value])
        for v, g in zip(variables, grads):
            out['%s_var_%s' % (tag, v.name)] = v.data.copy()
            out['%s_grad_%s' % (tag, v.name)] = g
        print('%-11s loss %.7f  |d rel_embeds|max %.3g' % (tag, value, np.abs(grads[1]).max()))
    np.savez_compressed(os.path.join(HERE, 'sea_graph.npz'), **out)


if __name__ == '__main__':
    main()
