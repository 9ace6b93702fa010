"""Golden loss and gradients of TransR's graph, from the REFERENCE's own code (models/trans/transr.py, run unmodified under
tests/golden/tf_shim.py through the helpers of make_tf_graph_golden.py).  Two cases, each one margin-loss batch:
  'tiny'   E = 14, R = 4, d = 5: the batch of tf_graphs.npz (transe_triple etc.);
  'd16'    E = 24, R = 5, d = 16: repeated relations and entities, one negative whose relation differs from its positive's.
The loss is evaluated in float64 at float32-representable variable values and its gradient w.r.t. ent_embeds, rel_embeds and
rel_matrix is taken by central finite differences.

Run in the build container only:  python tests/golden/make_transr_golden.py   -> tests/golden/transr_graph.npz
"""
import importlib
import os
import types

import numpy as np

from make_tf_graph_golden import HERE, fd_gradients, import_reference, quiet


def main():
    ref = import_reference()
    tf = ref.tf
    TransR = importlib.import_module('openea.models.trans.transr').TransR
    from openea_amd.run.default_args import get_args
    rng = np.random.RandomState(23)
    tiny_pos = np.array([[0, 1, 2], [3, 1, 4], [0, 0, 6], [7, 2, 0], [8, 3, 9]], np.int64)
    tiny_neg = np.array([[0, 1, 10], [11, 1, 4], [12, 0, 6], [7, 2, 5], [8, 3, 13]], np.int64)
    d16_pos = np.array([[0, 1, 2], [3, 1, 4], [0, 1, 6], [7, 2, 0], [8, 3, 9], [2, 1, 3], [10, 4, 11], [12, 1, 0],
                        [5, 0, 5], [13, 1, 14]], np.int64)
    d16_neg = np.array([[0, 1, 20], [21, 1, 4], [0, 1, 7], [7, 3, 1], [8, 3, 22], [2, 1, 23], [10, 4, 0], [12, 1, 15],
                        [16, 0, 5], [13, 1, 3]], np.int64)           # pair 3: the negative's relation (3) is not its positive's (2)
    out = {}
    for tag, n_ent, n_rel, d, pos, neg in (('tiny', 14, 4, 5, tiny_pos, tiny_neg), ('d16', 24, 5, 16, d16_pos, d16_neg)):
        del tf.VARIABLES[:]
        m = TransR()
        quiet(m.set_args, get_args('TransR', dim=d, output='/tmp/oea_golden/', training_data='synthetic/tiny/', dataset_division='f/'))
        m.set_kgs(types.SimpleNamespace(entities_num=n_ent, relations_num=n_rel))
        m._define_variables()
        m._define_embed_graph()
        variables = list(tf.VARIABLES)
        assert [v.name for v in variables] == ['ent_embeds', 'rel_embeds', 'rel_matrix'], [v.name for v in variables]
        for v in variables:                      # float32-representable values, moderately sized
            scale = 0.6 if v.name != 'rel_matrix' else 0.6 / np.sqrt(d)
            v.data = (rng.standard_normal(v.data.shape) * scale).astype(np.float32).astype(np.float64)
        feed = {m.pos_hs: pos[:, 0], m.pos_rs: pos[:, 1], m.pos_ts: pos[:, 2],
                m.neg_hs: neg[:, 0], m.neg_rs: neg[:, 1], m.neg_ts: neg[:, 2]}
        value = float(tf.evaluate(m.triple_loss, feed))
        grads = fd_gradients(tf, m.triple_loss, feed, variables)
        out[tag + '_pos'], out[tag + '_neg'] = pos, neg
        out[tag + '_shape'] = np.array([n_ent, n_rel, d])
        out[tag + '_margin'] = np.array([float(m.args.margin)])
        out[tag + '_loss'] = np.array([value])
        for v, g in zip(variables, grads):
            out['%s_var_%s' % (tag, v.name)] = v.data.copy()
            out['%s_grad_%s' % (tag, v.name)] = g
        print('%-6s loss %.6f  variables %s' % (tag, value, [v.name for v in variables]))
    np.savez_compressed(os.path.join(HERE, 'transr_graph.npz'), **out)


if __name__ == '__main__':
    main()
