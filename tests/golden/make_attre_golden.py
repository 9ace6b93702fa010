"""Golden values of AttrE from the REFERENCE's own code (approaches/attre.py: formatting_attr_triples, _define_variables,
_define_embed_graph; modules/train/batch.py: generate_attribute_triple_batch), run unmodified under tests/golden/tf_shim.py through
the helpers of make_tf_graph_golden.py.  What the stand-in lacks is supplied here, on the stand-in module, without editing it:
  unstack, reverse, slice, greater, subtract      numpy's, lazily where an operand is a graph node
  while_loop                                      a python loop over (cond, body): the loop variable `index` is a python number
                                                  there (tf.constant of an int), so the graph unrolls as the reference steps it
Cases:
  '<loss>_<norm>_d<dim>'   loss in margin / logistic / limited, norm L1 / L2, at (d = 5, L = 3) and (d = 16, L = 5): E = 14, A = 4,
      C = 7 characters, 8 value rows, 6 positives with k = 1 (margin) or k = 2 negatives.  The batch has an entity in two positives,
      negative heads that are other positives' heads, a value of all padding, a value with one character twice (and one thrice),
      two positives sharing an attribute.  triple_loss_ce and its central-difference gradients w.r.t. ent_embeds_ce, attr_embeds
      and char_embeds; joint_loss over all entities and its gradients w.r.t. ent_embeds and ent_embeds_ce (case 'joint_d<dim>').
      Gradients are taken at steps 1e-6 and 2e-6; '<case>_fd_err' = their largest difference (the truncation term) plus
      4 x 2^-52 |loss| / 1e-6 (the rounding of the two evaluations), which is what a comparison with them can resolve.
  'fmt_*'     formatting_attr_triples on make_kgs('tiny', attributes=True, string_values=True) at literal_len 5, as CHARACTERS:
      the cleaned value of every triple, the kept characters, and per triple the literal_len characters behind its ids ('' for
      id 0), so that no id order is compared.  'fmt_rare_*': the same on 320 hand-made values among which one character has a
      share below 0.0001, values with brackets, quotes, dots and underscores, an empty one and one that cleans to nothing.
  'batch_pos' the positives of every step of one epoch of generate_attribute_triple_batch(is_fixed_size=True) on the tiny lists
      at batch_size 1000, the topped-up last step included.
Losses are evaluated in float64 at float32-representable variable values.  Arrays only.

Run in the build container only:  python tests/golden/make_attre_golden.py   -> tests/golden/attre_graph.npz
"""
import importlib
import os
import sys
import types

import numpy as np

from make_tf_graph_golden import HERE, fd_gradients, import_reference, quiet

LOSSES = (('margin', 'margin-based', 1), ('logistic', 'logistic', 2), ('limited', 'limited', 2))
N_ENT, N_REL, N_ATTR, N_CHAR = 14, 4, 4, 7


def _extend_standin(tf):
    shim = sys.modules['tensorflow']
    is_node = lambda *xs: any(isinstance(x, tf.Node) for x in xs)       # noqa: E731

    def unstack(value, num=None, axis=0, name=None):
        return [tf.Node(lambda v, i=i: np.take(v, i, axis=axis), value) for i in range(num)]

    def reverse(tensor, axis, name=None):
        return tf.Node(lambda v: np.flip(v, axis=tuple(axis)), tensor)

    def slice_(input_, begin, size, name=None):
        assert all(s == -1 for s in size)
        begin = [int(b) for b in begin]
        return tf.Node(lambda v: v[tuple(slice(b, None) for b in begin)], input_)

    def greater(x, y, name=None):
        return tf.Node(np.greater, x, y) if is_node(x, y) else x > y

    def subtract(x, y, name=None):
        return tf.Node(np.subtract, x, y) if is_node(x, y) else x - y

    def while_loop(cond, body, loop_vars, **_):
        loop_vars = list(loop_vars)
        while cond(*loop_vars):
            loop_vars = list(body(*loop_vars))
        return loop_vars

    shim.unstack, shim.reverse, shim.slice = unstack, reverse, slice_
    shim.greater, shim.subtract, shim.while_loop = greater, subtract, while_loop


def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def _value_rows(L):
    rows = np.zeros((8, L), np.int64)
    rows[0, :3] = (1, 2, 3)
    rows[2, :3] = (4, 4, 5)            # one character twice
    rows[3, :2] = (6, 1)
    rows[4, 0] = 2
    rows[5, :3] = (3, 5, 6)
    rows[6, :3] = (1, 1, 1)
    rows[7, :3] = (5, 0, 2)            # padding inside a value
    if L > 3:
        rows[0, 3:] = 6
        rows[5, L - 1] = 4
    return rows                        # row 1: all padding


POS = np.array([[0, 1, 0], [3, 1, 1], [0, 0, 2], [7, 2, 3], [5, 3, 4], [9, 2, 6]], np.int64)
NEG_HEADS = np.array([[3, 10], [0, 7], [10, 0], [11, 3], [7, 13], [12, 9]], np.int64)      # [p, s]; NEG_HEADS[5, 1] is the positive's own head


def _char_feed(m, k):
    heads = NEG_HEADS[:, :k].reshape(-1)
    return {m.pos_es: POS[:, 0], m.pos_as: POS[:, 1], m.pos_vs: POS[:, 2], m.neg_es: heads,
            m.neg_as: np.repeat(POS[:, 1], k), m.neg_vs: np.repeat(POS[:, 2], k)}


def _two_step_gradients(tf, loss, feed, variables, value):
    g1 = fd_gradients(tf, loss, feed, variables, eps=1e-6)
    g2 = fd_gradients(tf, loss, feed, variables, eps=2e-6)
    diff = max(float(np.abs(a - b).max()) for a, b in zip(g1, g2))
    assert diff < 1e-6, "a hinge or an |x| of the batch lies on its kink: %g" % diff
    return g1, diff + 4 * 2.0 ** -52 * abs(value) / 1e-6


def _rare_values():
    """320 values of 40 characters over a small alphabet, one of them holding the only 'Q' (share 1 / 12,800 < 0.0001), and the
    cleaning cases of attre.py:27-34"""
    rng = np.random.RandomState(5)
    alphabet = "abcdefghij klmnop"
    vals = ["".join(alphabet[i] for i in rng.randint(0, len(alphabet), 40)) for _ in range(320)]
    vals[7] = "Q" + vals[7][1:]
    vals += ['New_York (city)', 'a.b,c-d"tail', '(all gone)', '', 'xy', 'trailing   (x)']
    return vals


def _as_characters(values, ids):
    L = ids.shape[1]
    return np.array([[v[i] if i < len(v) and row[i] != 0 else '' for i in range(L)] for v, row in zip(values, ids)], dtype='<U1')


def _format(attre, kgs, literal_len):
    """-> cleaned value per triple (KG1's then KG2's), kept characters (sorted), character rows, the two (e, a, value id) lists"""
    l1, l2, ids, size = attre.formatting_attr_triples(kgs, literal_len)
    long_len = 1 + max(len(v) for kg in (kgs.kg1, kgs.kg2) for (_, _, v) in kg.local_attribute_triples_list)
    _, _, ids_all, size_all = attre.formatting_attr_triples(kgs, long_len)
    assert size == size_all
    # the reference cleans in a function nested in formatting_attr_triples (no closure): run that very code object
    code = next(c for c in attre.formatting_attr_triples.__code__.co_consts
                if isinstance(c, types.CodeType) and c.co_name == 'clean_attribute_triples')
    clean = types.FunctionType(code, {})
    cleaned = [v for kg in (kgs.kg1, kgs.kg2) for (_, _, v) in clean(kg.local_attribute_triples_list)]
    ids, ids_all = np.asarray(ids, np.int64), np.asarray(ids_all, np.int64)
    kept = sorted({v[i] for v, row in zip(cleaned, ids_all) for i in range(len(v)) if row[i] != 0})
    assert len(kept) + 1 == size, (len(kept), size)
    return cleaned, kept, _as_characters(cleaned, ids), l1, l2


def main():
    ref = import_reference()
    tf = ref.tf
    _extend_standin(tf)
    attre = importlib.import_module('openea.approaches.attre')
    bat = importlib.import_module('openea.modules.train.batch')
    from openea_amd.run.default_args import get_args
    from openea_amd.modules.load.synth import make_kgs
    rng = np.random.RandomState(43)
    out = {'pos': POS, 'neg_heads': NEG_HEADS}
    common = dict(output='/tmp/oea_golden/', training_data='synthetic/tiny/', dataset_division='f/')

    for d, L in ((5, 3), (16, 5)):
        rows = _value_rows(L)
        out['value_chars_d%d' % d] = rows
        values = None
        for tag, loss, k in LOSSES:
            for norm in ('L1', 'L2'):
                del tf.VARIABLES[:]
                m = attre.AttrE()
                quiet(m.set_args, get_args('AttrE', dim=d, literal_len=L, loss=loss, loss_norm=norm, neg_triple_num=k,
                                           batch_size=len(POS), margin=1.5, pos_margin=0.8, neg_margin=2.5, **common))
                m.kgs = types.SimpleNamespace(entities_num=N_ENT, relations_num=N_REL, attributes_num=N_ATTR)
                m.value_id_char_ids, m.char_list_size = rows.tolist(), N_CHAR
                m._define_variables()
                m._define_embed_graph()
                variables = list(tf.VARIABLES)
                assert [v.data.shape for v in variables] == [(N_ENT, d), (N_REL, d), (N_ENT, d), (N_ATTR, d), (N_CHAR, d)]
                if values is None:
                    values = [_f32(rng.standard_normal(v.data.shape) * 0.6) for v in variables]
                    for name, v in zip(('ent_embeds', 'rel_embeds', 'ent_embeds_ce', 'attr_embeds', 'char_embeds'), values):
                        out['var_d%d_%s' % (d, name)] = v
                for v, data in zip(variables, values):
                    v.data = data.copy()
                case = '%s_%s_d%d' % (tag, norm, d)
                feed = _char_feed(m, k)
                value = float(tf.evaluate(m.triple_loss_ce, feed))
                grads, err = _two_step_gradients(tf, m.triple_loss_ce, feed, variables[2:], value)
                out[case + '_loss'], out[case + '_fd_err'] = np.array([value]), np.array([err])
                for name, g in zip(('ent_embeds_ce', 'attr_embeds', 'char_embeds'), grads):
                    out['%s_grad_%s' % (case, name)] = g
                print('%-18s loss %.6f  fd err %.2g' % (case, value, err))
        feed = {m.joint_ents: np.arange(N_ENT)}
        value = float(tf.evaluate(m.joint_loss, feed))
        grads, err = _two_step_gradients(tf, m.joint_loss, feed, [variables[0], variables[2]], value)
        case = 'joint_d%d' % d
        out[case + '_loss'], out[case + '_fd_err'] = np.array([value]), np.array([err])
        out[case + '_grad_ent_embeds'], out[case + '_grad_ent_embeds_ce'] = grads
        print('%-18s loss %.6f  fd err %.2g' % (case, value, err))
    out['margins'] = np.array([1.5, 0.8, 2.5])

    # ---- formatting and batches ---------------------------------------------------------------------------------------------------
    kgs = make_kgs('tiny', mode='sharing', seed=0, attributes=True, string_values=True)
    cleaned, kept, chars, l1, l2 = _format(attre, kgs, 5)
    out['fmt_cleaned'], out['fmt_kept'], out['fmt_chars'] = np.array(cleaned), np.array(kept, dtype='<U1'), chars
    out['fmt_triples'] = np.asarray(l1 + l2, np.int64)
    out['fmt_sizes'] = np.array([len(l1), len(l2)])
    assert any(len(v) > 5 for v in cleaned) and any(v == '' for v in cleaned)
    vals = _rare_values()
    half = len(vals) // 2
    small = types.SimpleNamespace(kg1=types.SimpleNamespace(local_attribute_triples_list=[(i, i % 3, v) for i, v in enumerate(vals[:half])]),
                                  kg2=types.SimpleNamespace(local_attribute_triples_list=[(i, i % 2, v) for i, v in enumerate(vals[half:])]))
    cleaned_s, kept_s, chars_s, _, _ = _format(attre, small, 5)
    assert 'Q' not in kept_s and chars_s[7, 0] == '' and cleaned_s[7][0] == 'Q'
    out['fmt_rare_values'], out['fmt_rare_cleaned'] = np.array(vals), np.array(cleaned_s)
    out['fmt_rare_kept'], out['fmt_rare_chars'] = np.array(kept_s, dtype='<U1'), chars_s
    batch_size = 1000
    steps = -(-(len(l1) + len(l2)) // batch_size)
    batches = []
    for step in range(steps):
        pos, _ = bat.generate_attribute_triple_batch(l1, l2, set(l1), set(l2), kgs.kg1.entities_list, kgs.kg2.entities_list, batch_size, step,
                                                     None, None, 1, True)
        assert len(pos) == batch_size
        batches.append(np.asarray(pos, np.int64))
    out['batch_pos'], out['batch_size'] = np.stack(batches), np.array([batch_size])
    print('formatting: %d + %d triples, %d kept characters; %d batches of %d' % (len(l1), len(l2), len(kept), steps, batch_size))
    np.savez_compressed(os.path.join(HERE, 'attre_graph.npz'), **out)


if __name__ == '__main__':
    main()
