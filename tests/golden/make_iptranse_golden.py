"""Golden losses, gradients and host-helper outputs of IPTransE, from the REFERENCE's own code (approaches/iptranse.py:
`_define_variables`, `_define_embed_graph` and `_define_alignment_graph` run unmodified under tests/golden/tf_shim.py through the
helpers of make_tf_graph_golden.py; `generate_2steps_path` -- pandas -- and `generate_triples_of_latent_ents` called as they are).
The stand-in lacks tf.maximum, which iptranse.py:165, 170 use: it is defined here.

Graph cases, each one batch of margin pairs (pos i, neg i), of path pairs (r_x, r_y, r | r', w) and of weighted alignment pairs:
  'ipt_d5'      E = 14, R = 6, d = 5
  'ipt_d16'     E = 24, R = 7, d = 16
  'ipt_d5_np0'  E = 14, R = 6, d = 5, the path batch empty
The path pairs of the first two hold one with r' == r, one with r_x == r_y, one inactive, a relation that only paths refer to and
one that nothing refers to; the alignment weights lie in [0.7, 1.0].  `train_loss` and `alignment_loss` are evaluated in float64
at float32-representable variable values, gradients w.r.t. ent_embeds and rel_embeds by central differences.  The variables of a
case are drawn with the first seed for which no hinge argument lies within 1e-3 of zero (central differences across the kink
would be wrong) and the path batch has its inactive pair.

Host helpers:
  'paths_tiny_*'   generate_2steps_path on KG1 of make_kgs('tiny', seed 0): the input triples and the sorted output rows
  'paths_hand_*'   the same on a hand-made list: two relations between the same (h, t), an (h, r) group with several tails, a path
                   of weight exactly 100 (kept) and one of weight 110 (dropped)
  'latent_*'       generate_triples_of_latent_ents on a small fixed pair of KGs

Run in the build container only:  python tests/golden/make_iptranse_golden.py   -> tests/golden/iptranse_graph.npz
"""
import importlib
import os
import types

import numpy as np

import tf_shim
from make_tf_graph_golden import HERE, fd_gradients, import_reference, quiet

tf_shim.maximum = tf_shim._op(np.maximum)

POS5 = [[0, 1, 2], [3, 1, 4], [0, 0, 6], [7, 2, 0], [8, 3, 9]]
NEG5 = [[0, 1, 10], [11, 1, 4], [12, 0, 6], [7, 2, 5], [8, 3, 13]]
# r_x, r_y, r, r', w: relation 4 occurs in paths only, relation 5 nowhere
PATH5 = [(0, 1, 2, 3, 1.0), (1, 1, 0, 2, 2.0), (2, 0, 3, 3, 4.0), (4, 0, 1, 2, 6.0), (3, 2, 0, 1, 100.0), (0, 2, 1, 4, 3.0),
         (1, 3, 2, 0, 12.0)]
ALIGN5 = ([[0, 1, 2], [7, 2, 0], [3, 0, 6], [8, 3, 9]], [[5, 1, 2], [7, 2, 11], [3, 0, 1], [13, 3, 9]],
          [0.75, 0.875, 0.96875, 0.8125])
POS16 = [[0, 1, 12], [3, 1, 4], [0, 0, 6], [7, 2, 0], [8, 3, 9], [15, 4, 20], [21, 0, 3]]
NEG16 = [[0, 1, 10], [11, 1, 4], [12, 0, 6], [7, 2, 5], [8, 3, 13], [15, 4, 23], [22, 0, 3]]
# relation 5 occurs in paths only, relation 6 nowhere
PATH16 = [(0, 1, 2, 3, 1.0), (2, 2, 4, 1, 2.0), (3, 0, 1, 1, 9.0), (5, 0, 1, 2, 6.0), (3, 2, 0, 4, 100.0), (0, 4, 1, 5, 3.0),
          (1, 3, 2, 0, 20.0), (4, 4, 3, 0, 1.0), (0, 1, 2, 4, 5.0)]
ALIGN16 = ([[0, 1, 12], [7, 2, 0], [3, 0, 6], [8, 3, 9], [15, 4, 20]], [[5, 1, 12], [7, 2, 11], [3, 0, 1], [13, 3, 9], [15, 4, 2]],
           [0.75, 0.875, 0.96875, 0.8125, 1.0])
CASES = (
    ('ipt_d5', 14, 6, 5, POS5, NEG5, PATH5, ALIGN5),
    ('ipt_d16', 24, 7, 16, POS16, NEG16, PATH16, ALIGN16),
    ('ipt_d5_np0', 14, 6, 5, POS5, NEG5, [], ALIGN5),
)
NAMES = ['ent_embeds', 'rel_embeds']


def _l2n(x):
    return x / np.sqrt(np.maximum((x * x).sum(1, keepdims=True), 1e-12))


def hinge_arguments(ent, rel, pos, neg, paths, margin):
    """every hinge argument of the case's three batches (triples, paths, alignment pairs share this form)"""
    e, r = _l2n(ent), _l2n(rel)
    score = lambda t: ((e[t[:, 0]] + r[t[:, 1]] - e[t[:, 2]]) ** 2).sum(1)
    tri = score(pos) + margin - score(neg)
    if len(paths) == 0:
        return tri, np.zeros(0)
    p = np.asarray([q[:4] for q in paths], np.int64)
    base = r[p[:, 0]] + r[p[:, 1]]
    return tri, ((base - r[p[:, 2]]) ** 2).sum(1) + margin - ((base - r[p[:, 3]]) ** 2).sum(1)


def path_cases_hand():
    """h = 0 -r0-> 10 tails (1..10); 1 -r1-> 10 tails (11..20): weight 100; 2 -r1-> 11 tails (21..31): weight 110; closing triples
    (0, r2, 11), (0, r3, 11) -- two relations between the same (h, t) --, (0, r2, 21); and a short chain 40 -r4-> 41 -r5-> 42"""
    tri = [(0, 0, m) for m in range(1, 11)]
    tri += [(1, 1, t) for t in range(11, 21)]
    tri += [(2, 1, t) for t in range(21, 32)]
    tri += [(0, 2, 11), (0, 3, 11), (0, 2, 21)]
    tri += [(40, 4, 41), (41, 5, 42), (40, 6, 42), (40, 4, 43), (43, 5, 42)]
    return tri


def sorted_rows(paths):
    a = np.asarray([[float(x) for x in p] for p in paths], np.float64).reshape(-1, 4)
    return a[np.lexsort(a.T[::-1])] if len(a) else a


def main():
    ref = import_reference()
    tf = ref.tf
    mod = importlib.import_module('openea.approaches.iptranse')
    from openea_amd.modules.load.synth import make_kgs
    from openea_amd.run.default_args import get_args
    out = {}
    for tag, n_ent, n_rel, d, pos, neg, paths, align in CASES:
        del tf.VARIABLES[:]
        m = mod.IPTransE()
        quiet(m.set_args, get_args('IPTransE', dim=d, output='/tmp/oea_golden/', training_data='synthetic/tiny/', dataset_division='f/'))
        m.set_kgs(types.SimpleNamespace(entities_num=n_ent, relations_num=n_rel))
        m._define_variables()
        m._define_embed_graph()
        m._define_alignment_graph()
        variables = list(tf.VARIABLES)
        assert [v.name for v in variables] == NAMES, [v.name for v in variables]
        pos, neg = np.asarray(pos, np.int64), np.asarray(neg, np.int64)
        apos, aneg, aw = np.asarray(align[0], np.int64), np.asarray(align[1], np.int64), np.asarray(align[2], np.float64)
        margin = float(m.args.margin)
        for seed in range(1000):                 # the first seed that keeps every hinge argument off the kink
            rng = np.random.RandomState(seed)
            vals = [(rng.standard_normal(v.data.shape) * 0.6).astype(np.float32).astype(np.float64) for v in variables]
            tri, pth = hinge_arguments(vals[0], vals[1], pos, neg, paths, margin)
            ali, _ = hinge_arguments(vals[0], vals[1], apos, aneg, [], margin)
            args = np.concatenate([tri, pth, ali])
            ok = np.abs(args).min() > 1e-3 and (tri > 0).any() and (tri < 0).any() and (ali > 0).sum() >= 2
            if len(paths):
                ok = ok and (pth < 0).any() and (pth > 0).sum() >= 4
            if ok:
                break
        else:
            raise AssertionError('no seed')
        assert np.abs(args).min() > 1e-3
        for v, x in zip(variables, vals):
            v.data = x
        pw = np.asarray([q[4] for q in paths], np.float64)
        pp = np.asarray([q[:4] for q in paths], np.int64).reshape(-1, 4)
        if len(paths):
            assert (pp[:, 2] == pp[:, 3]).any() and (pp[:, 0] == pp[:, 1]).any()
            used_tri, used_path = set(pos[:, 1]) | set(neg[:, 1]), set(pp.reshape(-1))
            assert used_path - used_tri and set(range(n_rel)) - used_path - used_tri
        feed = {m.pos_hs: pos[:, 0], m.pos_rs: pos[:, 1], m.pos_ts: pos[:, 2], m.neg_hs: neg[:, 0], m.neg_rs: neg[:, 1],
                m.neg_ts: neg[:, 2], m.pos_rx: pp[:, 0], m.pos_ry: pp[:, 1], m.pos_r: pp[:, 2], m.neg_rx: pp[:, 0],
                m.neg_ry: pp[:, 1], m.neg_r: pp[:, 3], m.path_weight: pw}
        afeed = {m.new_ph: apos[:, 0], m.new_pr: apos[:, 1], m.new_pt: apos[:, 2], m.new_nh: aneg[:, 0], m.new_nr: aneg[:, 1],
                 m.new_nt: aneg[:, 2], m.tr_weight: aw}
        out[tag + '_shape'] = np.array([n_ent, n_rel, d])
        out[tag + '_consts'] = np.array([margin, float(m.args.path_parm)])
        out[tag + '_seed'] = np.array([seed])
        out[tag + '_pos'], out[tag + '_neg'] = pos, neg
        out[tag + '_paths'], out[tag + '_path_weight'] = pp, pw
        out[tag + '_align_pos'], out[tag + '_align_neg'], out[tag + '_align_weight'] = apos, aneg, aw
        out[tag + '_path_args'] = pth
        for v in variables:
            out['%s_var_%s' % (tag, v.name)] = v.data.copy()
        for name, loss, fd in (('train', m.train_loss, feed), ('align', m.alignment_loss, afeed)):
            value = float(tf.evaluate(loss, fd))
            grads = fd_gradients(tf, loss, fd, variables)
            out['%s_%s_loss' % (tag, name)] = np.array([value])
            for v, g in zip(variables, grads):
                out['%s_%s_grad_%s' % (tag, name, v.name)] = g
            print('%-11s %-5s loss %.7f  |d ent|max %.3g  |d rel|max %.3g' % (tag, name, value, np.abs(grads[0]).max(),
                                                                             np.abs(grads[1]).max()))

    tiny = make_kgs('tiny', mode='swapping', seed=0).kg1.relation_triples_list
    for tag, tri in (('paths_tiny', tiny), ('paths_hand', path_cases_hand())):
        rows = sorted_rows(quiet(mod.generate_2steps_path, list(tri)))
        out[tag + '_triples'] = np.asarray(tri, np.int64)
        out[tag + '_rows'] = rows
        print('%-11s %d triples -> %d paths, weights %g .. %g' % (tag, len(tri), len(rows), rows[:, 3].min(), rows[:, 3].max()))
    hand = out['paths_hand_rows']
    assert (hand[:, 3] == 100.0).any() and hand[:, 3].max() == 100.0

    t1 = [(0, 0, 1), (0, 1, 2), (3, 0, 0), (4, 1, 0), (1, 0, 2)]
    t2 = [(10, 2, 11), (12, 2, 10), (10, 3, 13), (11, 3, 12)]
    from openea_amd.modules.load.kg import _grouped
    kgs = types.SimpleNamespace(
        kg1=types.SimpleNamespace(rt_dict=_grouped(t1, 0, (1, 2)), hr_dict=_grouped(t1, 2, (0, 1))),
        kg2=types.SimpleNamespace(rt_dict=_grouped(t2, 0, (1, 2)), hr_dict=_grouped(t2, 2, (0, 1))))
    ents1, ents2, ws = [0, 1, 5], [10, 11, 12], [0.75, 0.875, 0.8125]
    latent = quiet(mod.generate_triples_of_latent_ents, kgs, ents1, ents2, ws)
    out['latent_triples1'], out['latent_triples2'] = np.asarray(t1, np.int64), np.asarray(t2, np.int64)
    out['latent_ents1'], out['latent_ents2'], out['latent_ws'] = np.asarray(ents1), np.asarray(ents2), np.asarray(ws)
    out['latent_rows'] = sorted_rows(latent)
    print('latent      %d triples' % len(latent))
    np.savez_compressed(os.path.join(HERE, 'iptranse_graph.npz'), **out)


if __name__ == '__main__':
    main()
