"""AttrE without a GPU: the float64 restatement (_attre_ref.py) against the reference's own graph (golden/attre_graph.npz, written
by golden/make_attre_golden.py), the closed-form composition weights, the formatting and batch-layout mirrors of approaches/attre.py
against the reference's outputs, the head sampler's restatement, the shipped args and the refusals."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _attre_ref as ref  # noqa: E402
from openea_amd.approaches import attre  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "attre_graph.npz"))
LOSSES = (("margin", "margin-based", 1), ("logistic", "logistic", 2), ("limited", "limited", 2))
CASES = [(tag, loss, k, norm, d) for d in (5, 16) for tag, loss, k in LOSSES for norm in ("L1", "L2")]


def golden_batch(loss, k, norm, d):
    margin, pos_margin, neg_margin = GOLD["margins"]
    return dict(pos=GOLD["pos"], neg_heads=GOLD["neg_heads"][:, :k].reshape(-1), value_chars=GOLD["value_chars_d%d" % d], k=k, loss=loss,
                l1=norm == "L1", margin=margin, pos_margin=pos_margin, neg_margin=neg_margin, balance=1.0, ent_l2n=True, attr_l2n=True,
                char_l2n=True)


def golden_tables(d, names=("ent_embeds_ce", "attr_embeds", "char_embeds")):
    return [GOLD["var_d%d_%s" % (d, n)] for n in names]


@pytest.mark.parametrize("tag,loss,k,norm,d", CASES)
def test_restatement_equals_reference_graph(tag, loss, k, norm, d):
    case = "%s_%s_d%d" % (tag, norm, d)
    value, grads = ref.char_grads(golden_tables(d), golden_batch(loss, k, norm, d))
    assert abs(value - GOLD[case + "_loss"][0]) <= 1e-12 * abs(value)
    err = GOLD[case + "_fd_err"][0]
    for name, g in zip(("ent_embeds_ce", "attr_embeds", "char_embeds"), grads):
        dev = np.abs(g - GOLD["%s_grad_%s" % (case, name)]).max()
        print("%s %s: gradient off by %.3g (central-difference error %.3g)" % (case, name, dev, err))
        assert dev <= err


@pytest.mark.parametrize("d", [5, 16])
def test_joint_restatement_equals_reference_graph(d):
    ent, ce = golden_tables(d, ("ent_embeds", "ent_embeds_ce"))
    value, grads = ref.joint_grads(ent, ce, True)
    assert abs(value - GOLD["joint_d%d_loss" % d][0]) <= 1e-12 * abs(value)
    for name, g in zip(("ent_embeds", "ent_embeds_ce"), grads):
        assert np.abs(g - GOLD["joint_d%d_grad_%s" % (d, name)]).max() <= GOLD["joint_d%d_fd_err" % d][0]


@pytest.mark.parametrize("L", [1, 2, 5, 10])
def test_closed_form_weights_equal_the_reversed_prefix_loop(L):
    assert np.abs(ref.weights(L) - ref.weights_loop(L)).max() <= 1e-15 * L
    if L == 5:
        assert np.allclose(ref.weights(5), [2.2833, 1.2833, 0.7833, 0.45, 0.2], atol=5e-5)


# ---- formatting --------------------------------------------------------------------------------------------------------------------
def _kgs_of(values):
    import types
    half = len(values) // 2
    side = lambda vs, m: types.SimpleNamespace(local_attribute_triples_list=[(i, i % m, v) for i, v in enumerate(vs)])    # noqa: E731
    return types.SimpleNamespace(kg1=side(values[:half], 3), kg2=side(values[half:], 2))


def _check_formatting(kgs, literal_len, cleaned, kept, chars):
    l1, l2, ids, size = attre.formatting_attr_triples(kgs, literal_len)
    values = [attre.clean_value(v) for kg in (kgs.kg1, kgs.kg2) for (_, _, v) in kg.local_attribute_triples_list]
    assert values == list(cleaned)
    ours = attre.kept_characters(values)
    assert sorted(ours) == list(kept) and size == len(kept) + 1
    assert ids.shape == (len(values), literal_len) and ids.dtype == np.int32 and ids.min() >= 0 and ids.max() < size
    table = np.array([""] + ours, dtype="<U1")
    assert (table[ids] == chars).all()
    assert [t[2] for t in l1 + l2] == list(range(len(values)))                # a value id of its own per triple
    assert [t[:2] for t in l1] == [t[:2] for t in kgs.kg1.local_attribute_triples_list]
    return values, ours, ids


def test_formatting_equals_the_reference_on_tiny():
    from openea_amd.modules.load.synth import make_kgs
    kgs = make_kgs("tiny", mode="sharing", seed=0, attributes=True, string_values=True)
    values, ours, ids = _check_formatting(kgs, 5, GOLD["fmt_cleaned"], GOLD["fmt_kept"], GOLD["fmt_chars"])
    assert any(len(v) > 5 for v in values)                                     # longer than literal_len: cut
    empty = [i for i, v in enumerate(values) if v == ""]
    assert empty and (ids[empty] == 0).all()                                   # empty after cleaning: all padding
    counts = {}
    for v in set(values):
        for ch in v:
            counts[ch] = counts.get(ch, 0) + 1
    order = [(-counts[ch], ord(ch)) for ch in ours]
    assert order == sorted(order)                                              # descending count, then code point
    l1, l2, _, _ = attre.formatting_attr_triples(kgs, 5)
    assert (np.asarray(l1 + l2) == GOLD["fmt_triples"]).all()


def test_formatting_drops_a_rare_character_and_cleans():
    vals = [str(v) for v in GOLD["fmt_rare_values"]]
    values, ours, ids = _check_formatting(_kgs_of(vals), 5, GOLD["fmt_rare_cleaned"], GOLD["fmt_rare_kept"], GOLD["fmt_rare_chars"])
    assert values[7][0] == "Q" and "Q" not in ours and ids[7, 0] == 0 and ids[7, 1] != 0        # dropped: id 0 in place
    assert values[-6:] == ["New York", "abc d", "", "", "xy", "trailing"]


# ---- layout ------------------------------------------------------------------------------------------------------------------------
def test_layout_equals_the_recorded_batches():
    n1, n2 = (int(v) for v in GOLD["fmt_sizes"])
    b = int(GOLD["batch_size"][0])
    slot, b1, steps = attre.attr_batch_layout(n1, n2, b)
    got = GOLD["fmt_triples"][slot].reshape(steps, b, 3)
    assert got.shape == GOLD["batch_pos"].shape and (got == GOLD["batch_pos"]).all()
    assert b1 == int(n1 / (n1 + n2) * b)
    last = slot.reshape(steps, b)[-1]
    assert (last[:b1] < n1).all() and (last[b1:] >= n1).all() and 0 in last and n1 in last       # topped up from the heads


def test_layout_refuses_a_batch_larger_than_a_side():
    slot, b1, steps = attre.attr_batch_layout(10, 1000, 600)
    assert (b1, steps, len(slot)) == (5, 2, 1200)
    with pytest.raises(ValueError):
        attre.attr_batch_layout(3, 5, 20)               # b = 7 + 13 of lists of 3 + 5
    with pytest.raises(ValueError):
        attre.attr_batch_layout(100, 4, 200)            # b2 = 8 > 4


# ---- sampler -----------------------------------------------------------------------------------------------------------------------
def _sides(list0, list1, n_ent):
    poss = []
    for lst in (list0, list1):
        p = np.full(n_ent, -1, np.int32)
        p[np.asarray(lst)] = np.arange(len(lst), dtype=np.int32)
        poss.append(p)
    return (np.asarray(list0, np.int32), np.asarray(list1, np.int32)), poss


def test_head_sampler_restatement():
    lists, poss = _sides([4, 0, 2], [1, 3, 5, 6, 7], 8)
    rng = np.random.RandomState(3)
    n, k, split = 4000, 3, 2500
    pos = np.zeros((n, 3), np.int32)
    pos[:split, 0] = rng.choice(lists[0], split)
    pos[split:, 0] = rng.choice(lists[1], n - split)
    out = ref.sample_heads(pos, split, k, lists, poss, seed=77, step=5).reshape(n, k)
    assert (out != pos[:, :1]).all()                                            # never the head
    assert np.isin(out[:split], lists[0]).all() and np.isin(out[split:], lists[1]).all()
    for h in lists[0]:                                                          # three entities: both others, about evenly
        drawn = out[:split][pos[:split, 0] == h].reshape(-1)
        others = [e for e in lists[0] if e != h]
        share = np.array([(drawn == e).mean() for e in others])
        assert share.sum() == 1.0 and np.abs(share - 0.5).max() < 0.05
    again = ref.sample_heads(pos, split, k, lists, poss, seed=77, step=5).reshape(n, k)
    other = ref.sample_heads(pos, split, k, lists, poss, seed=77, step=6).reshape(n, k)
    assert (again == out).all() and (other != out).any()
    part = ref.sample_heads(pos[100:], split - 100, k, lists, poss, seed=77, step=5, pos_offset=100).reshape(-1, k)
    assert (part == out[100:]).all()                                            # a pure function of the position


# ---- args and refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", ["15K", "100K"])
def test_default_args_equal_the_shipped_files(scale):
    from openea_amd.run.default_args import get_args
    shipped = json.load(open(os.path.join(HERE, "golden", "attre_args_%s.json" % scale)))
    ours = get_args("AttrE", scale).__dict__
    for k, v in shipped.items():
        assert k in ours and ours[k] == v, (k, v, ours.get(k))
    assert set(ours) == set(shipped)


@pytest.mark.parametrize("over", [dict(dim=129), dict(optimizer="Adam"), dict(optimizer="Adadelta"), dict(neg_triple_num=2),
                                  dict(neg_sampling="truncated"), dict(literal_len=33)])
def test_refusals_come_before_any_table(over):
    from openea_amd.run.default_args import get_args
    m = attre.AttrE()
    m.set_args(get_args("AttrE", output="/tmp/oea_attre_cpu/", training_data="synthetic/tiny/", dataset_division="f/", **over))
    with pytest.raises(NotImplementedError):
        m.init()
    assert m.ent_embeds is None and m.char_embeds is None


def test_exported():
    import openea_amd.approaches as ap
    assert ap.AttrE is attre.AttrE
