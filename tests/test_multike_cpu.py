"""MultiKE without a GPU: the float64 restatements of tests/_multike_ref.py against the reference's own graphs
(golden/multike_graph.npz, written by golden/make_multike_golden.py: the reference's conv, _define_variables and _define_*_graph under
the TF stand-in, gradients by central differences), the host functions against golden/multike.json, the weight-vector form against
add_weights' per-triple weights, the batch layout against the reference's slicing, the args and the refusals.

The fixture rests on the assumptions M1-M4 of _multike_ref.py about TF 1.x (the padding of an even 'same' kernel, the batch
norm's inference mode and positional axis, l2_normalize without an axis, the flat order): the stand-in's layers state them once
more, independently of the restatement, but nothing here can run TensorFlow to pin them."""
import json
import os

import numpy as np
import pytest

import _multike_ref as ref
from openea_amd.approaches import multi_ke as mk
from openea_amd.approaches import predicate_alignmnet as pa

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "multike_graph.npz")
CASES = ("multike_d6", "multike_d16")
FD_TOL = 2e-6            # central differences at eps = 1e-6 in float64: truncation eps^2 f''' / 6 and rounding 1e-16 f / eps, both ~1e-10
                         # of a gradient of order one; the bound leaves four orders of room and still sees a missing factor or term


def fixture_case(z, tag):
    E, R, A, L, d, B = (int(x) for x in z[tag + "_shape"])
    tables = {name: z["%s_var_%s" % (tag, name)] for name in ("rv_ent_embeds", "rel_embeds", "av_ent_embeds", "attr_embeds", "ent_embeds")}
    sets = [{name: z["%s_var_cnn%d_%s" % (tag, i, name)] for name in ref.VARS} for i in range(4)]
    return dict(d=d, tables=tables, sets=sets, lit=z[tag + "_lit"], names=z[tag + "_names"], pos=z[tag + "_pos"], neg=z[tag + "_neg"],
                att=z[tag + "_att"], att_w=z[tag + "_att_w"], rel_w=z[tag + "_rel_w"], ents=z[tag + "_ents"])


def _close(got, want, what):
    off = np.abs(np.asarray(got) - want).max()
    scale = max(np.abs(want).max(), 1e-30)
    print("%s: off by %.3g of its largest entry %.3g" % (what, off / scale, scale))
    assert off <= FD_TOL * scale + 1e-9, what


def _check(z, tag, loss_name, loss, grads):
    want = float(z["%s_%s" % (tag, loss_name)][0])
    print("%s %s: %.12g (fixture %.12g)" % (tag, loss_name, loss, want))
    assert abs(loss - want) <= 1e-10 * abs(want)
    keys = [k for k in z.files if k.startswith("%s_%s_grad_" % (tag, loss_name))]
    assert sorted(k.split("_grad_")[1] for k in keys) == sorted(grads), (keys, sorted(grads))
    for label, g in grads.items():
        _close(g, z["%s_%s_grad_%s" % (tag, loss_name, label)], "%s %s d/d %s" % (tag, loss_name, label))


def _cnn_labels(k, grads):
    return {"cnn%d_%s" % (k, name): grads[name] for name in ref.VARS}


@pytest.mark.parametrize("tag", CASES)
def test_attribute_view_graph(tag):
    """multi_ke.py:532-555: the weighted net on av_ent_embeds, the unweighted one on ent_embeds, 0.5 |f - name|^2"""
    z = np.load(GOLDEN)
    c = fixture_case(z, tag)
    t = c["tables"]
    l0, g0, ge0, ga0, _, c0 = ref.cnn_loss_grads(c["sets"][0], t["av_ent_embeds"], t["attr_embeds"], c["lit"], c["att"], c["att_w"])
    l1, g1, ge1, ga1, _, c1 = ref.cnn_loss_grads(c["sets"][1], t["ent_embeds"], t["attr_embeds"], c["lit"], c["att"])
    l2, gy, _ = ref.pull_term(t["ent_embeds"], c["names"], c["att"][:, 0], 0.5, l2n=(True, False))
    assert min(c0["raw"].min(), c1["raw"].min()) > 1e-3 and min(c0["tn"], c1["tn"]) > 1e-3          # no clamp is active
    grads = dict(av_ent_embeds=ge0, attr_embeds=ga0 + ga1, ent_embeds=ge1 + ref.through_l2n(t["ent_embeds"], gy))
    grads.update(_cnn_labels(0, g0))
    grads.update(_cnn_labels(1, g1))
    _check(z, tag, "attribute_loss", l0 + l1 + l2, grads)


@pytest.mark.parametrize("tag", CASES)
def test_cross_kg_attribute_graphs(tag):
    """multi_ke.py:573-586 (factor 2, unweighted, the third parameter set) and :604-621 (weighted, the fourth)"""
    z = np.load(GOLDEN)
    c = fixture_case(z, tag)
    t = c["tables"]
    l, g, ge, ga, _, _ = ref.cnn_loss_grads(c["sets"][2], t["av_ent_embeds"], t["attr_embeds"], c["lit"], c["att"], None, 2.0)
    _check(z, tag, "ckge_attribute_loss", l, dict(av_ent_embeds=ge, attr_embeds=ga, **_cnn_labels(2, g)))
    l, g, ge, ga, _, _ = ref.cnn_loss_grads(c["sets"][3], t["av_ent_embeds"], t["attr_embeds"], c["lit"], c["att"], c["att_w"])
    _check(z, tag, "ckga_attribute_loss", l, dict(av_ent_embeds=ge, attr_embeds=ga, **_cnn_labels(3, g)))


@pytest.mark.parametrize("tag", CASES)
def test_relation_view_graph(tag):
    """multi_ke.py:502-530: the logistic loss on (rv, rel) and the four cross-view terms on the positives"""
    z = np.load(GOLDEN)
    c = fixture_case(z, tag)
    t = c["tables"]
    f, rv, rel, pos = t["ent_embeds"], t["rv_ent_embeds"], t["rel_embeds"], c["pos"]
    l0, ge, gr = ref.logistic_term(rv, rel, pos, c["neg"])
    l1, gf1, grv1, gr1 = ref.cross_term(f, rv, rel, pos)
    l2, grv2, gf2, gr2 = ref.cross_term(rv, f, rel, pos)
    l3, gf3, _ = ref.pull_term(f, c["names"], pos[:, 0], 0.5, l2n=(True, False))
    l4, gf4, _ = ref.pull_term(f, c["names"], pos[:, 2], 0.5, l2n=(True, False))
    grads = dict(rv_ent_embeds=ref.through_l2n(rv, ge + grv1 + grv2), rel_embeds=ref.through_l2n(rel, gr + gr1 + gr2),
                 ent_embeds=ref.through_l2n(f, gf1 + gf2 + gf3 + gf4))
    _check(z, tag, "relation_loss", l0 + l1 + l2 + l3 + l4, grads)


@pytest.mark.parametrize("tag", CASES)
def test_cross_kg_relation_and_common_space_graphs(tag):
    """multi_ke.py:559-571 (2 positive_loss), :588-602 (2 sum w softplus) and :625-638 (an entity twice in the batch counts twice)"""
    z = np.load(GOLDEN)
    c = fixture_case(z, tag)
    t = c["tables"]
    f, rv, av, rel, pos = t["ent_embeds"], t["rv_ent_embeds"], t["av_ent_embeds"], t["rel_embeds"], c["pos"]
    l, ga, gb, gr = ref.cross_term(rv, rv, rel, pos, 2.0)
    _check(z, tag, "ckge_relation_loss", l, dict(rv_ent_embeds=ref.through_l2n(rv, ga + gb), rel_embeds=ref.through_l2n(rel, gr)))
    l, ga, gb, gr = ref.wsoft_term(rv, rv, rel, pos, None, 2.0, triple_weight=c["rel_w"])
    _check(z, tag, "ckgp_relation_loss", l, dict(rv_ent_embeds=ref.through_l2n(rv, ga + gb), rel_embeds=ref.through_l2n(rel, gr)))
    ids = c["ents"]
    assert len(set(ids.tolist())) < len(ids)
    l0, g0, _ = ref.pull_term(f, c["names"], ids, 1.0, l2n=(True, False))
    l1, g1, grv = ref.pull_term(f, rv, ids)
    l2, g2, gav = ref.pull_term(f, av, ids)
    _check(z, tag, "cross_name_loss", l0 + l1 + l2, dict(ent_embeds=ref.through_l2n(f, g0 + g1 + g2), rv_ent_embeds=ref.through_l2n(rv, grv),
                                                         av_ent_embeds=ref.through_l2n(av, gav)))


def test_the_restatement_handles_both_clamps():
    """a zero dense layer makes t = 0: the block norm's clamp is active, y = t / 1e-6 and the loss is sum softplus(|h|^2) = B softplus(1)"""
    P = ref.cnn_problem(1, 5, 4, nets=1)
    p = P["params"][0]
    p["W"], p["bd"] = np.zeros_like(p["W"]), np.zeros_like(p["bd"])
    loss, g, ge, ga, _, c = ref.cnn_loss_grads(p, P["ents"][0], P["attr"], P["lit"], P["batch"])
    assert c["tn"] == 0.0 and abs(loss - 5 * np.log1p(np.e)) < 1e-12
    assert np.abs(g["K1"]).max() == 0.0 and np.abs(ga).max() == 0.0 and np.abs(g["bd"]).max() > 0      # nothing flows through W = 0
    want = (-2.0 / (1.0 + np.exp(-1.0))) * c["u"][P["batch"][:, 0]] * 1e6            # dL/dt = dL/dy / 1e-6, dL/dy = -2 sigmoid(1) h
    assert np.abs(g["bd"] - want.sum(0)).max() <= 1e-9 * np.abs(want).max()


# ---- host functions ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    return json.load(open(os.path.join(HERE, "golden", "multike.json")))


def test_clear_attribute_triples(host):
    cleaned, numbers, strings = mk.clear_attribute_triples([tuple(t) for t in host["clear_in"]])
    assert sorted([list(t) for t in cleaned]) == host["clear_out"]
    assert sorted(numbers) == host["clear_numbers"] and sorted(strings) == host["clear_strings"]
    assert all(a != 3 for (_, a, _) in cleaned) and all(a != 4 for (_, a, _) in cleaned)      # a rare attribute; values with 'http'
    assert mk.is_number("1.5") and mk.is_number("½") and not mk.is_number("1.5.2")


def test_zoom_and_weights(host):
    for w, mb, want in host["zoom"]:
        assert pa.zoom_weight(w, mb) == want
    links = [tuple(x) for x in host["links"]]
    t1, t2 = [tuple(t) for t in host["triples1"]], [tuple(t) for t in host["triples2"]]
    w1, w2, s1, s2 = pa.add_weights(links, t1, t2, host["min_w_before"])
    assert [list(t) for t in w1] == host["weighted1"] and [list(t) for t in w2] == host["weighted2"]
    assert s1 == set(w1) and s2 == set(w2)
    sup1, sup2 = pa.generate_sup_predicate_triples(links, t1, t2)
    assert [list(t) for t in sup1] == host["sup1"] and [list(t) for t in sup2] == host["sup2"]
    # the vector form: a triple's weight is its predicate's entry
    vec = pa.weight_vector(links, sorted({p for (_, p, _) in t1}), sorted({p for (_, p, _) in t2}), 8, host["min_w_before"])
    for (_, p, _, w) in w1 + w2:
        assert vec[p] == w
    sup = pa.sup_weight_vector(links, 8)
    for (_, p, _, w) in sup1 + sup2:
        assert sup[p] == w
    with pytest.raises(ValueError):
        pa.weight_vector([(0, 5, 0.95)], [0], [0, 5], 8, 0.8)          # id 0 in both KGs: 0.875 in one, 0.2 in the other


def test_init_predicate_alignment(host):
    n1, n2 = host["names1"], host["names2"]
    k1, k2 = sorted(n1), sorted(n2)
    ratios = pa.name_ratios([n1[k] for k in k1], [n2[k] for k in k2], on_device=False)
    pairs, latent = pa.init_predicate_alignment(n1, n2, host["init_sim"], ratios)
    assert sorted([list(p) for p in pairs]) == host["init_pairs"]
    assert sorted([[a, b, s] for (a, b), s in latent.items()]) == host["init_latent"]
    assert len(pairs) >= 1 and len(latent) > len(pairs)


def test_find_predicate_alignment_by_embedding(host):
    found = pa.find_predicate_alignment_by_embedding(np.asarray(host["embed"]), host["list1"], host["list2"])
    got = sorted([[i, j, s] for (i, j), s in found.items()])
    assert [g[:2] for g in got] == [w[:2] for w in host["found"]] and len(got) >= 2
    assert np.abs(np.array([g[2] for g in got]) - np.array([w[2] for w in host["found"]])).max() <= 1e-12


# ---- batches -------------------------------------------------------------------------------------------------------------------
def _reference_batches(list1, list2, batch_size, steps):
    """generate_attribute_triple_batch's slices (multi_ke.py:280-291, batch.py:48-53), restated"""
    b1 = int(len(list1) / (len(list1) + len(list2)) * batch_size)
    b2 = batch_size - b1
    out = []
    for step in range(steps):
        part = []
        for triples, b in ((list1, b1), (list2, b2)):
            start = step * b
            end = min(start + b, len(triples))
            part += triples[start:end]
        out.append(part)
    return out


@pytest.mark.parametrize("n1,n2,batch,steps", [(7, 5, 6, 3), (100, 37, 20, 7), (10, 90, 30, 5), (5, 5, 4, 1), (9, 0, 4, 3)])
def test_attribute_batch_layout_equals_the_reference_slices(n1, n2, batch, steps):
    list1, list2 = [("a", i) for i in range(n1)], [("b", i) for i in range(n2)]
    slot, offsets = mk.attribute_batch_layout(n1, n2, batch, steps)
    both = list1 + list2
    want = _reference_batches(list1, list2, batch, steps)
    for s in range(steps):
        assert [both[i] for i in slot[offsets[s]:offsets[s + 1]]] == want[s], s
    assert offsets[-1] == len(slot)


# ---- args, refusals, literal vectors -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", ["15K", "100K"])
def test_default_args_equal_the_shipped_files(scale):
    from openea_amd.run.default_args import get_args
    shipped = json.load(open(os.path.join(HERE, "golden", "multike_args_%s.json" % scale)))
    ours = get_args("MultiKE", scale).__dict__
    for k, v in shipped.items():
        assert k in ours and ours[k] == v, (k, v, ours.get(k))
    assert set(ours) - set(shipped) == {"literal_vectors_path"}


def _model(encoder=True, **over):
    from openea_amd.run.default_args import get_args
    m = mk.MultiKE()
    m.set_args(get_args("MultiKE", output="/tmp/oea_multike_cpu/", training_data="synthetic/tiny/", dataset_division="f/", **over))
    if encoder:
        m.literal_encoder = lambda literals: np.zeros((len(literals), m.args.dim), np.float32)
    return m


@pytest.mark.parametrize("over", [dict(dim=129), dict(optimizer="Adam"), dict(optimizer="Adagrad"), dict(neg_sampling="truncated")])
def test_refusals_come_before_any_table(over):
    m = _model(**over)
    with pytest.raises(NotImplementedError):
        m.init()
    assert m.ent_embeds is None and m.rel_embeds is None and not hasattr(m, "literal_list")


def test_no_literal_source_and_no_space_mapping():
    m = _model(encoder=False)
    with pytest.raises(NotImplementedError):
        m.init()
    assert m.ent_embeds is None
    with pytest.raises(NotImplementedError):
        _model()._define_space_mapping_graph()
    with pytest.raises(NotImplementedError):
        _model().train_shared_space_mapping_1epo(1, [])


def test_missing_literals_are_counted(tmp_path):
    from openea_amd.modules.load import synth
    path = str(tmp_path / "vectors.npz")
    np.savez(path, literals=np.array(["only this"]), vectors=np.zeros((1, 100), np.float32))
    m = _model(encoder=False, literal_vectors_path=path)
    m.set_kgs(synth.make_kgs("tiny", mode="swapping", seed=0, attributes=True, string_values=True))
    m.entities = m.kgs.kg1.entities_set | m.kgs.kg2.entities_set
    m.entity_local_name_dict = m._get_local_name_by_name_triple()
    with pytest.raises(ValueError, match=r"\d+ of \d+ literals have no vector"):
        m._generate_literal_vectors()


def test_literal_vectors():
    from openea_amd.modules.load import synth
    v = synth.literal_vectors(["a b", "b a", "a b c d e f", "a b c d e g", "", "a"], 8, seed=3)
    assert v.shape == (6, 8) and v.dtype == np.float32
    assert np.array_equal(v[0], v[1]) and np.array_equal(v[2], v[3]) and not np.array_equal(v[0], v[5])       # a mean; five words
    assert np.array_equal(v, synth.literal_vectors(["a b", "b a", "a b c d e f", "a b c d e g", "", "a"], 8, seed=3))
    assert not np.array_equal(v, synth.literal_vectors(["a b", "b a", "a b c d e f", "a b c d e g", "", "a"], 8, seed=4))
    assert np.abs(v[4]).max() > 0


def test_exported():
    import openea_amd.approaches as ap
    assert ap.MultiKE is mk.MultiKE
    from openea_amd import ops
    assert ops.MULTIKE_MAX_DIM == 128 and len(ops.MULTIKE_VARS) == 8
    assert [int(np.prod(s)) for s in ops.multike_cnn_shapes(100)] == [100, 100, 16, 2, 32, 2, 400 * 100, 100]
