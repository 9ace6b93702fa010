"""IPTransE without a GPU: a float64 restatement of its two losses (CPU torch autograd, rows GATHERED as the reference does, not
through the Gram matrix the device uses) against the reference's own graphs (tests/golden/iptranse_graph.npz,
make_iptranse_golden.py), the reference steps the GPU tests (test_iptranse_gpu.py) hold the device to, the host helpers against
the reference's own outputs, and the argument contract."""
import os
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "iptranse_graph.npz")
CASES = ["ipt_d5", "ipt_d16", "ipt_d5_np0"]


def _l2n_rows(x):
    """tf.nn.l2_normalize(x, 1)"""
    return x * torch.rsqrt(torch.clamp((x * x).sum(1, keepdim=True), min=1e-12))


def _ids(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.long)


def _score(e, r, tri):
    tri = _ids(tri).reshape(-1, 3)
    return ((e[tri[:, 0]] + r[tri[:, 1]] - e[tri[:, 2]]) ** 2).sum(1)


def path_hinge_arguments(r, batch):
    """|x + y - r|^2 + margin - |x + y - r'|^2 per path pair, rows of the normalised table r"""
    p = _ids(batch["paths"]).reshape(-1, 3)
    base = r[p[:, 0]] + r[p[:, 1]]
    return ((base - r[p[:, 2]]) ** 2).sum(1) + batch["margin"] - ((base - r[_ids(batch["neg_rel"])]) ** 2).sum(1)


def iptranse_loss(ent, rel, batch, l2n=(True, True)):
    """iptranse.py:158-181 in float64.  batch: pos, neg int [n, 3]; paths int [m, 3] = (r_x, r_y, r), neg_rel int [m],
    weight [m]; margin, path_parm.  -> (loss, triple hinge arguments, path hinge arguments)"""
    e = _l2n_rows(ent) if l2n[0] else ent
    r = _l2n_rows(rel) if l2n[1] else rel
    tri = _score(e, r, batch["pos"]) + batch["margin"] - _score(e, r, batch["neg"])
    loss = torch.clamp(tri, min=0).sum()
    pth = torch.zeros(0, dtype=ent.dtype)
    if len(batch["paths"]):
        pth = path_hinge_arguments(r, batch)
        inv_w = 1.0 / torch.as_tensor(np.asarray(batch["weight"], np.float64))
        loss = loss + batch["path_parm"] * (inv_w * torch.clamp(pth, min=0)).sum()
    return loss, tri, pth


def weighted_pair_loss(ent, rel, batch, l2n=(True, True)):
    """iptranse.py:167-170 in float64.  batch: pos, neg int [n, 3], weight [n], margin -> (loss, hinge arguments)"""
    e = _l2n_rows(ent) if l2n[0] else ent
    r = _l2n_rows(rel) if l2n[1] else rel
    arg = _score(e, r, batch["pos"]) + batch["margin"] - _score(e, r, batch["neg"])
    w = torch.as_tensor(np.asarray(batch["weight"], np.float64))
    return (w * torch.clamp(arg, min=0)).sum(), arg


def _grads(fn, ent, rel, batch):
    vs = [torch.tensor(np.asarray(v, np.float64), requires_grad=True) for v in (ent, rel)]
    out = fn(vs[0], vs[1], batch)
    grads = torch.autograd.grad(out[0], vs, allow_unused=True)
    grads = [np.zeros_like(np.asarray(v, np.float64)) if g is None else g.numpy() for g, v in zip(grads, (ent, rel))]
    return float(out[0].detach()), grads, [o.detach().numpy() for o in out[1:]]


def _apply(tables, accs, grads, lr, optimizer):
    for p, g, a in zip(tables, grads, accs):
        if optimizer == "Adagrad":          # tf.train.AdagradOptimizer: no epsilon, accumulator from 0.1
            a += g * g
            p -= lr * g / np.sqrt(a)
        else:
            assert optimizer == "SGD"
            p -= lr * g


def iptranse_reference_step(tables, accs, batch, lr, optimizer):
    """one step of train_loss's optimiser in place (float64): tables = [ent, rel], accs = their Adagrad accumulators (ignored
    for SGD).  -> (batch loss, [gradients], smallest |hinge argument| of the batch)"""
    loss, grads, args = _grads(iptranse_loss, tables[0], tables[1], batch)
    _apply(tables, accs, grads, lr, optimizer)
    return loss, grads, float(min(np.abs(a).min() if a.size else np.inf for a in args))


def weighted_pair_reference_step(tables, accs, batch, lr, optimizer):
    """the same for alignment_loss"""
    loss, grads, args = _grads(weighted_pair_loss, tables[0], tables[1], batch)
    _apply(tables, accs, grads, lr, optimizer)
    return loss, grads, float(np.abs(args[0]).min()) if args[0].size else np.inf


def fixture_case(z, case):
    """-> tables [ent, rel], the training batch, the alignment batch"""
    tables = [z["%s_var_%s" % (case, n)] for n in ("ent_embeds", "rel_embeds")]
    margin, path_parm = (float(x) for x in z[case + "_consts"])
    pp = z[case + "_paths"]
    train = dict(pos=z[case + "_pos"], neg=z[case + "_neg"], paths=pp[:, :3], neg_rel=pp[:, 3], weight=z[case + "_path_weight"],
                 margin=margin, path_parm=path_parm)
    align = dict(pos=z[case + "_align_pos"], neg=z[case + "_align_neg"], weight=z[case + "_align_weight"], margin=margin)
    return tables, train, align


@pytest.mark.parametrize("which", ["train", "align"])
@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_reference_graph(case, which):
    z = np.load(GOLDEN)
    (ent, rel), train, align = fixture_case(z, case)
    loss, grads, _ = _grads(iptranse_loss if which == "train" else weighted_pair_loss, ent, rel, train if which == "train" else align)
    ref_loss = z["%s_%s_loss" % (case, which)][0]
    assert abs(loss - ref_loss) <= 1e-6 * abs(ref_loss)
    for name, g in zip(("ent_embeds", "rel_embeds"), grads):
        ref = z["%s_%s_grad_%s" % (case, which, name)]
        assert g.shape == ref.shape
        assert np.abs(ref).max() > 0, name
        assert np.abs(g - ref).max() <= 1e-6 * np.abs(ref).max(), name


@pytest.mark.parametrize("which", ["train", "align"])
@pytest.mark.parametrize("case", CASES)
def test_reference_step_under_sgd_moves_by_the_gradient(case, which):
    z = np.load(GOLDEN)
    tables, train, align = fixture_case(z, case)
    lr = 0.01
    mine = [t.copy() for t in tables]
    step = iptranse_reference_step if which == "train" else weighted_pair_reference_step
    loss, _, nearest = step(mine, [None, None], train if which == "train" else align, lr, "SGD")
    assert nearest > 1e-3                              # the maker's condition: no hinge argument near the kink
    assert abs(loss - z["%s_%s_loss" % (case, which)][0]) <= 1e-6 * loss
    for name, before, after in zip(("ent_embeds", "rel_embeds"), tables, mine):
        ref = z["%s_%s_grad_%s" % (case, which, name)]
        assert np.abs((before - after) / lr - ref).max() <= 1e-6 * np.abs(ref).max(), name


def test_fixture_covers_the_cases():
    z = np.load(GOLDEN)
    assert [tuple(z[c + "_shape"]) for c in CASES] == [(14, 6, 5), (24, 7, 16), (14, 6, 5)]
    assert len(z["ipt_d5_np0_paths"]) == 0
    for case in CASES[:2]:
        pp, args = z[case + "_paths"], z[case + "_path_args"]
        n_rel = int(z[case + "_shape"][1])
        assert (pp[:, 2] == pp[:, 3]).any() and (pp[:, 0] == pp[:, 1]).any()         # r' == r; r_x == r_y
        assert (args < 0).any() and (args > 0).any()                                # one inactive
        in_tri = set(z[case + "_pos"][:, 1]) | set(z[case + "_neg"][:, 1])
        in_path = set(pp.reshape(-1))
        assert in_path - in_tri                                                     # a relation only paths refer to
        assert set(range(n_rel)) - in_path - in_tri                                 # one nothing refers to
        assert np.abs(args[pp[:, 2] == pp[:, 3]] - z[case + "_consts"][0]).max() < 1e-12        # r' == r: the margin, active
    for case in CASES:
        w = z[case + "_align_weight"]
        assert (w >= 0.7).all() and (w <= 1.0).all()
        for k in ("_path_weight", "_align_weight", "_var_ent_embeds", "_var_rel_embeds"):
            assert np.array_equal(z[case + k], z[case + k].astype(np.float32).astype(np.float64)), k


def _sorted_rows(paths):
    a = np.asarray([[float(x) for x in p] for p in paths], np.float64).reshape(-1, 4)
    return a[np.lexsort(a.T[::-1])] if len(a) else a


@pytest.mark.parametrize("tag", ["paths_tiny", "paths_hand"])
def test_generate_2steps_path_equals_the_reference(tag, capsys):
    from openea_amd.approaches.iptranse import generate_2steps_path
    z = np.load(GOLDEN)
    ref = z[tag + "_rows"]
    paths = generate_2steps_path([tuple(int(x) for x in t) for t in z[tag + "_triples"]])
    assert "num of path: %d" % len(ref) in capsys.readouterr().out
    assert all(isinstance(p[0], int) and isinstance(p[3], float) for p in paths)
    assert np.array_equal(_sorted_rows(paths), ref)


def test_tiny_input_is_the_synthetic_kg():
    from openea_amd.modules.load.synth import make_kgs
    z = np.load(GOLDEN)
    assert np.array_equal(np.asarray(make_kgs("tiny", mode="swapping", seed=0).kg1.relation_triples_list), z["paths_tiny_triples"])


def test_hand_made_list_keeps_weight_100_and_drops_110():
    z = np.load(GOLDEN)
    rows = z["paths_hand_rows"]
    assert (rows[:, 3] == 100.0).sum() == 2 and rows[:, 3].max() == 100.0        # two relations close the same (h, t)
    assert len(rows) == 4


def test_path_mining_prunes_large_groups_before_the_join():
    """a hub whose (h, r) group has 150 tails: none of its edges can be in a path of weight < 101, with or without the pruning"""
    from openea_amd.approaches.iptranse import two_step_path_arrays
    tri = [(0, 0, t) for t in range(1, 151)] + [(t, 1, 200) for t in range(1, 151)] + [(0, 2, 200), (300, 3, 0), (300, 4, 5)]
    paths, w = two_step_path_arrays(tri)
    # (300, r3, 0), (0, r0, 5) closes with (300, r4, 5): weight 1 x 150 -> dropped; nothing else closes
    assert len(paths) == 0 and len(w) == 0
    assert two_step_path_arrays([])[0].shape == (0, 3)


def test_latent_triples_equal_the_reference(capsys):
    from openea_amd.approaches.iptranse import generate_triples_of_latent_ents
    from openea_amd.modules.load.kg import _grouped
    z = np.load(GOLDEN)
    t1, t2 = ([tuple(int(x) for x in t) for t in z[k]] for k in ("latent_triples1", "latent_triples2"))
    kgs = types.SimpleNamespace(
        kg1=types.SimpleNamespace(rt_dict=_grouped(t1, 0, (1, 2)), hr_dict=_grouped(t1, 2, (0, 1))),
        kg2=types.SimpleNamespace(rt_dict=_grouped(t2, 0, (1, 2)), hr_dict=_grouped(t2, 2, (0, 1))))
    got = generate_triples_of_latent_ents(kgs, z["latent_ents1"].tolist(), z["latent_ents2"].tolist(), z["latent_ws"].tolist())
    assert "newly triples: %d" % len(z["latent_rows"]) in capsys.readouterr().out
    assert isinstance(got, set) and np.array_equal(_sorted_rows(got), z["latent_rows"])


def test_batch_helpers_keep_their_contracts():
    import random
    from openea_amd.approaches.iptranse import generate_neg_paths, generate_neg_triples_w, generate_triple_batch
    random.seed(3)
    paths = [(0, 1, 2, 4.0), (3, 3, 1, 1.0)] * 50
    neg = generate_neg_paths(paths, [7, 8, 9])
    assert [p[:2] for p in neg] == [p[:2] for p in paths] and {p[2] for p in neg} == {7, 8, 9} and all(len(p) == 3 for p in neg)
    triples = {(h, 0, h + 1, 0.5 + h / 64.0) for h in range(30)}
    ents = list(range(100, 140))
    pos, negs = generate_triple_batch(triples, 20, ents)
    assert len(pos) == 20 == len(set(pos)) and set(pos) <= triples
    pos_all, neg_all = generate_triple_batch(triples, 50, ents)
    assert len(pos_all) == 30 and set(pos_all) == triples
    heads = tails = 0
    for (h, r, t, w), (h2, r2, t2, w2) in zip(pos_all + pos, neg_all + negs):
        assert r2 == r and w2 == w and (h2 == h) != (t2 == t)
        assert (h2 if t2 == t else t2) in ents
        heads += t2 == t
        tails += h2 == h
    assert heads > 5 and tails > 5
    assert len(generate_neg_triples_w(pos, ents)) == len(pos)


# run/args/iptranse_args_15K.json
SHIPPED = dict(training_data="../../datasets/", output="../../output/results/", dataset_division="721_5fold", embedding_module="IPTransE",
               alignment_module="sharing", search_module="greedy", dim=100, init="normal", ent_l2_norm=True, rel_l2_norm=True,
               loss_norm="L2", learning_rate=0.01, optimizer="Adagrad", max_epoch=2000, batch_size=5000, margin=1.5, path_parm=0.1,
               neg_sampling="uniform", neg_triple_num=1, batch_threads_num=2, test_threads_num=4, ordered=True, start_valid=100,
               eval_freq=10, stop_metric="hits1", eval_metric="inner", csls=10, top_k=[1, 5, 10, 50], is_save=True, eval_norm=False,
               sim_th=0.7, bp_freq=100)
# what run/args/iptranse_args_100K.json changes
SHIPPED_100K = dict(batch_size=20000, batch_threads_num=3, test_threads_num=10)


@pytest.mark.parametrize("scale", ["15K", "100K"])
def test_args_match_the_shipped_run_configs(scale):
    from openea_amd.run.default_args import get_args
    a = get_args("IPTransE", scale)
    expect = dict(SHIPPED, **(SHIPPED_100K if scale == "100K" else {}))
    for k, v in expect.items():
        assert getattr(a, k) == v, k
    assert set(a.__dict__) == set(expect)


@pytest.mark.parametrize("bad", [dict(alignment_module="mapping"), dict(init="xavier"), dict(neg_sampling="truncated"),
                                 dict(optimizer="Adam"), dict(eval_metric="euclidean"), dict(loss_norm="L1"),
                                 dict(ent_l2_norm=False), dict(rel_l2_norm=False), dict(margin=0.0), dict(neg_triple_num=2),
                                 dict(sim_th=0.0)])
def test_check_args_rejects_each_asserted_key(bad):
    """iptranse.py:136-149"""
    from openea_amd.approaches import IPTransE
    from openea_amd.run.default_args import get_args
    m = IPTransE()
    m.args = get_args("IPTransE")
    m._check_args()
    m.args = get_args("IPTransE", **bad)
    with pytest.raises(AssertionError):
        m._check_args()


def test_no_path_in_either_kg_is_announced_once_and_gives_p_zero(capsys):
    """the reference divides by zero there (iptranse.py:77); here the path half is skipped"""
    from openea_amd.approaches import IPTransE
    m = IPTransE()
    m.paths1, m.paths2 = [], []
    assert m._path_batch_size(18) == 0 and m._path_batch_size(18) == 0
    out = capsys.readouterr().out
    assert out.count("no two-step relation path") == 1 and "plain TransE" in out
    m.paths1, m.paths2 = [(0, 1, 2, 1.0)] * 966, [(0, 1, 2, 1.0)] * 544
    assert m._path_batch_size(18) == 83
    assert capsys.readouterr().out == ""


def test_init_refuses_more_than_one_rank():
    """a torch.distributed group: NotImplementedError before any path is mined or table made (no device is touched)"""
    from openea_amd.approaches import IPTransE
    from openea_amd.run.default_args import get_args
    m = IPTransE()
    m.args = get_args("IPTransE")
    m.kgs = types.SimpleNamespace(entities_num=10, relations_num=2)
    m._dist_group = lambda: object()
    with pytest.raises(NotImplementedError, match="one GPU"):
        m.init()
    assert m.ent_embeds is None and m.paths1 is None
