"""Golden losses and gradients of JAPE's three graphs, from the REFERENCE's own code (approaches/jape.py: _define_variables,
_define_embed_graph and _define_sim_graph; approaches/attr2vec.py: _define_variables and _define_embed_graph, run unmodified under
tests/golden/tf_shim.py through the helpers of make_tf_graph_golden.py), and the outputs of the reference's host functions
get_kgs_popular_attributes, generate_training_data and get_ent_embeds_from_attributes (with the selected attributes, and with
three of them only, which leaves zero rows) on the synthetic 'tiny' KG pair with attributes.  What the stand-in lacks is supplied
here, on the stand-in module, without editing it:
  trainable_variables   every Variable (jape.py:96 filters them by name)
  nn.nce_loss           as in make_proje_golden.py: num_true = 1, accidental hits kept, log Q subtracted, sigmoid cross entropy summed
                        over the true and the sampled columns; the candidates come from the seeded numpy restatement of the
                        log-uniform sampler (tests/test_proje_cpu.py) and are recorded
Cases, each one batch:
  'attr_d5'   A = 14, d = 5,  B = 6,  S = 4        'attr_d16'  A = 40, d = 16, B = 10, S = 8
      a repeated input, a repeated label, a label that is among the samples, one pair with input == label
  'triple_d5' E = 14, R = 4, d = 5, k = 2, neg_alpha 0.1: entities repeat, a negative shares rows with its positive, one triple h == t
  'sim_d5'    E = 14, d = 5, four reference entities a side, a 3 x 4 block of the similarity matrix with an all-zero row
Losses are evaluated in float64 at float32-representable variable values; gradients are central differences.  Arrays only.

Run in the build container only:  python tests/golden/make_jape_golden.py   -> tests/golden/jape_graph.npz
"""
import importlib
import os
import sys
import types

import numpy as np

from make_tf_graph_golden import HERE, REPO, fd_gradients, import_reference, quiet

sys.path.insert(0, os.path.join(REPO, 'tests'))
from test_proje_cpu import log_q, log_uniform_reference  # noqa: E402

SEED = 20190719


def _extend_standin(tf, record):
    shim = sys.modules['tensorflow']

    def nce_loss(weights, biases, labels, inputs, num_sampled, num_classes, **_):
        sampled, num_tries, _ = log_uniform_reference(num_classes, num_sampled, SEED, 0)
        record['sampled'], record['num_tries'] = sampled, num_tries

        def fn(w, b, lab, x):
            t = np.asarray(lab, np.int64).reshape(-1)
            true = (x * w[t]).sum(1) + b[t] - log_q(t, num_tries, num_classes)
            samp = x @ w[sampled].T + b[sampled] - log_q(sampled, num_tries, num_classes)
            xent = lambda v, z: np.maximum(v, 0) - v * z + np.log1p(np.exp(-np.abs(v)))        # noqa: E731
            return xent(true, 1.0) + xent(samp, 0.0).sum(1)
        return tf.Node(fn, weights, biases, labels, inputs)

    shim.nn.nce_loss = nce_loss
    shim.trainable_variables = lambda: list(tf.VARIABLES)


def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def _attr_batch(tag, sampled):
    hit = int(sampled[0])
    if tag == 'attr_d5':
        return np.array([[0, 1], [3, 1], [0, 2], [7, hit], [8, 9], [5, 5]], np.int64)
    return np.array([[0, 1], [3, 1], [0, 6], [7, hit], [8, 9], [2, 4], [10, 11], [12, 0], [5, 5], [0, 30]], np.int64)


def main():
    ref = import_reference()
    tf = ref.tf
    record = {}
    _extend_standin(tf, record)
    a2v = importlib.import_module('openea.approaches.attr2vec')
    JAPE = importlib.import_module('openea.approaches.jape').JAPE
    from openea_amd.run.default_args import get_args
    from openea_amd.modules.load.synth import make_kgs
    rng = np.random.RandomState(41)
    out = {}
    common = dict(output='/tmp/oea_golden/', training_data='synthetic/tiny/', dataset_division='f/')

    # ---- Attr2Vec's graph ---------------------------------------------------------------------------------------------------
    for tag, n_attr, d, n_b, n_s in (('attr_d5', 14, 5, 6, 4), ('attr_d16', 40, 16, 10, 8)):
        del tf.VARIABLES[:]
        m = a2v.Attr2Vec()
        quiet(m.set_args, get_args('JAPE', dim=d, batch_size=n_b, **common))
        m.kgs = types.SimpleNamespace(attributes_num=n_attr)
        m.num_sampled_negs = n_s
        m._define_variables()
        m._define_embed_graph()
        variables = list(tf.VARIABLES)
        assert len(variables) == 3 and variables[0].data.shape == (n_attr, d) and variables[2].data.shape == (n_attr,)
        sampled, num_tries = record['sampled'], record['num_tries']
        pairs = _attr_batch(tag, sampled)
        assert len(pairs) == n_b and pairs.max() < n_attr
        variables[0].data = _f32(rng.standard_normal((n_attr, d)) * 0.6)
        variables[1].data = _f32(rng.standard_normal((n_attr, d)) * 0.6)
        variables[2].data = _f32(rng.standard_normal(n_attr) * 0.3)
        feed = {m.train_inputs: pairs[:, 0]}
        # attr2vec.py:120 rebinds self.train_labels to the reshaped node: feed the placeholder under it
        feed[m.train_labels.inputs[0]] = pairs[:, 1]
        value = float(tf.evaluate(m.loss, feed))
        grads = fd_gradients(tf, m.loss, feed, variables)
        out[tag + '_pairs'] = pairs
        out[tag + '_sampled'] = np.asarray(sampled, np.int64)
        out[tag + '_num_tries'] = np.array([num_tries], np.int64)
        out[tag + '_shape'] = np.array([n_attr, d, n_b, n_s])
        out[tag + '_loss'] = np.array([value])
        for name, v, g in zip(('embeds', 'nce_weights', 'nce_biases'), variables, grads):
            out['%s_var_%s' % (tag, name)] = v.data.copy()
            out['%s_grad_%s' % (tag, name)] = g
        print('%-10s loss %.6f  sampled %s  num_tries %d' % (tag, value, list(sampled), num_tries))

    # ---- JAPE's triple and similarity graphs ----------------------------------------------------------------------------------
    del tf.VARIABLES[:]
    n_ent, n_rel, d, k = 14, 4, 5, 2
    m = JAPE()
    quiet(m.set_args, get_args('JAPE', dim=d, neg_triple_num=k, sub_mat_size=3, **common))
    m.kgs = types.SimpleNamespace(entities_num=n_ent, relations_num=n_rel)
    m.ref_entities1, m.ref_entities2 = [2, 5, 9, 12], [3, 6, 10, 13]
    m._define_variables()
    m._define_embed_graph()
    m._define_sim_graph()
    variables = list(tf.VARIABLES)
    assert [v.data.shape for v in variables] == [(n_ent, d), (n_rel, d)], [v.name for v in variables]
    for v in variables:
        v.data = _f32(rng.standard_normal(v.data.shape) * 0.6)
    pos = np.array([[0, 1, 2], [3, 1, 4], [0, 0, 6], [7, 2, 0], [5, 3, 5]], np.int64)
    neg = np.array([[0, 1, 10], [11, 1, 2], [12, 1, 4], [3, 1, 3], [0, 0, 9], [13, 0, 6], [7, 2, 1], [7, 3, 0], [5, 3, 8],
                    [2, 3, 5]], np.int64)
    feed = {m.pos_hs: pos[:, 0], m.pos_rs: pos[:, 1], m.pos_ts: pos[:, 2], m.neg_hs: neg[:, 0], m.neg_rs: neg[:, 1], m.neg_ts: neg[:, 2]}
    out['triple_d5_pos'], out['triple_d5_neg'] = pos, neg
    out['triple_d5_shape'] = np.array([n_ent, n_rel, d, k])
    out['triple_d5_neg_alpha'] = np.array([float(m.args.neg_alpha)])
    out['triple_d5_loss'] = np.array([float(tf.evaluate(m.triple_loss, feed))])
    for name, v, g in zip(('ent_embeds', 'rel_embeds'), variables, fd_gradients(tf, m.triple_loss, feed, variables)):
        out['triple_d5_var_' + name] = v.data.copy()
        out['triple_d5_grad_' + name] = g
    idx = np.array([3, 0, 2])
    sim = _f32(np.array([[0.97, 0.0, 0.0, 0.99], [0.0, 0.0, 0.0, 0.0], [0.0, 0.96, 1.0, 0.0], [0.0, 0.0, 0.98, 0.0]]))
    feed = {m.entities1: np.asarray(m.ref_entities1)[idx], m.attr_sim_mat_place: sim[idx]}
    out['sim_d5_ref1'], out['sim_d5_ref2'] = np.asarray(m.ref_entities1), np.asarray(m.ref_entities2)
    out['sim_d5_mat'], out['sim_d5_idx'] = sim, idx
    out['sim_d5_beta'] = np.array([float(m.args.attr_sim_mat_beta)])
    out['sim_d5_loss'] = np.array([float(tf.evaluate(m.sim_loss, feed))])
    out['sim_d5_empty_row_loss'] = np.array([float(tf.evaluate(m.sim_loss, {m.entities1: np.asarray(m.ref_entities1)[[1, 1, 1]],
                                                                            m.attr_sim_mat_place: sim[[1, 1, 1]]}))])
    print('triple_d5  loss %.6f   sim_d5 loss %.8f (three empty rows %.8f)'
          % (out['triple_d5_loss'][0], out['sim_d5_loss'][0], out['sim_d5_empty_row_loss'][0]))

    # ---- the host functions on a tiny KG pair ------------------------------------------------------------------------------------
    kgs = make_kgs('tiny', mode='sharing', seed=0, attributes=True)
    sel1, sel2, sel = quiet(a2v.get_kgs_popular_attributes, kgs, 0.9)
    data = quiet(a2v.generate_training_data, kgs, threshold=0.9)
    attr_embeds = rng.standard_normal((kgs.attributes_num, 6)).astype(np.float32)
    ent_mat = quiet(a2v.get_ent_embeds_from_attributes, kgs, attr_embeds, sel)
    out['host_selected1'], out['host_selected2'] = np.array(sorted(sel1), np.int32), np.array(sorted(sel2), np.int32)
    out['host_selected'] = np.array(sorted(sel), np.int32)
    out['host_training_data'] = np.asarray(data, np.int32).reshape(-1, 2)
    out['host_attr_embeds'] = attr_embeds
    out['host_ent_mat'] = np.asarray(ent_mat, np.float32)
    # a selection of three attributes leaves most entities without any: their rows are zero (attr2vec.py:63-70)
    few = set(sorted(sel)[:3])
    ent_mat_few = np.asarray(quiet(a2v.get_ent_embeds_from_attributes, kgs, attr_embeds, few), np.float32)
    assert 0 < int((np.abs(ent_mat_few).sum(1) == 0).sum()) < len(ent_mat_few)
    out['host_selected_few'], out['host_ent_mat_few'] = np.array(sorted(few), np.int32), ent_mat_few
    print('host: %d + %d -> %d selected attributes of %d, %d training pairs, entity matrix %s (%d zero rows)'
          % (len(sel1), len(sel2), len(sel), kgs.attributes_num, len(data), ent_mat.shape, int((np.abs(ent_mat).sum(1) == 0).sum())))
    np.savez_compressed(os.path.join(HERE, 'jape_graph.npz'), **out)


if __name__ == '__main__':
    main()
