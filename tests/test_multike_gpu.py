"""MultiKE on the device: oea_multike_cnn_step and oea_multike_rows (csrc/multike_step.hip) against the float64 restatements of
tests/_multike_ref.py (assumptions M1-M4 there), run to run, and the approach end to end."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import _multike_ref as ref  # noqa: E402

U24 = 2.0 ** -24
EDGE_SHAPES = [(3, 2), (5, 3), (33, 75), (70, 64), (65, 65), (40, 100), (130, 128), (257, 127)]


# ---- the CNN step on the device ----------------------------------------------------------------------------------------------------
def _params_dev(p, d, dev):
    from openea_amd import ops
    out = []
    for name in ref.VARS:
        out.append(ops.to_table(p[name], dev=dev) if name == "W" else ops.to_vec(p[name].reshape(-1), dev))
    return out


def _setup(P, dev, max_n, lr=0.01):
    from openea_amd import ops
    d = P["d"]
    ents = [ops.to_table(e, dev=dev) for e in P["ents"]]
    attr, lit = ops.to_table(P["attr"], dev=dev), ops.to_table(P["lit"], dev=dev)
    ld = attr.shape[1]
    dummy = torch.zeros((3, ld), device=dev)
    n_rel = [attr.shape[0], 3]
    rels = [attr, dummy]
    wss = [ops.step_workspace(e.shape[0], n_rel[k], ld, dev) for k, e in enumerate(ents)]
    params = [_params_dev(p, d, dev) for p in P["params"]]
    nets = [ops.multike_net(params[k], ents[k], wss[k], n_rel[k], weighted=(k == 0), factor=P["factors"][k]) for k in range(len(ents))]
    cfg = ops.make_step_cfg(loss="positive", optimizer="SGD", lr=lr, ent_l2_norm=True, rel_l2_norm=False)
    return dict(d=d, ents=ents, attr=attr, lit=lit, rels=rels, wss=wss, params=params, nets=nets, cfg=cfg, lr=lr,
                aw=ops.to_vec(P["aw"], dev), ws=ops.multike_cnn_workspace(d, ld, max_n, dev),
                loss=torch.zeros(1, dtype=torch.float64, device=dev), empty=torch.zeros((0, 3), dtype=torch.int32, device=dev))


def _cnn(S, batch, phase):
    from openea_amd import ops
    ops.multike_cnn_step(S["nets"], S["attr"], S["lit"], S["d"], batch, S["aw"], S["lr"], S["ws"], S["loss"], phase=phase)


def _apply(S):
    from openea_amd import ops
    sink = torch.zeros(1, dtype=torch.float64, device=S["loss"].device)
    for k, e in enumerate(S["ents"]):
        ops.triple_step(e, None, S["rels"][k], None, S["d"], S["empty"], None, S["cfg"], S["wss"][k], sink, phase=ops.PHASE_APPLY)


def _variables(S):
    return S["ents"] + [S["attr"]] + [t for p in S["params"] for t in p]


def _check_grad_phase(P, what):
    """PHASE_GRAD against the restatement: loss within 2e-5 relative, every gradient within 1e-3 of max |ref|, nothing moved;
    then the engine's apply phase under SGD with lr = 1 gives the table gradients: before - after."""
    from openea_amd import ops
    dev = ops.device()
    d, B = P["d"], len(P["batch"])
    loss_ref, per, g_attr, caches = ref.cnn_problem_grads(P)
    for c in caches:                              # no clamp is active
        assert c["raw"].min() >= 1e-3 and c["tn"] >= 1e-3
    S = _setup(P, dev, B, lr=1.0)
    before = [t.clone() for t in _variables(S)]
    batch = ops.to_ids(P["batch"], dev)
    _cnn(S, batch, ops.PHASE_GRAD)
    loss = float(S["loss"].item())
    print("%s: loss %.9g (restatement %.9g, relative %.3g)" % (what, loss, loss_ref, abs(loss - loss_ref) / loss_ref))
    assert abs(loss - loss_ref) <= 2e-5 * loss_ref
    assert all(torch.equal(a, b) for a, b in zip(_variables(S), before))
    for k in range(len(P["ents"])):
        got = ops.multike_cnn_grads(S["ws"], k)
        for name, g in zip(ref.VARS, got):
            r = per[k][0][name]
            g = g.cpu().numpy().astype(np.float64)
            if name == "W":
                assert np.abs(g[:, d:]).max(initial=0.0) == 0.0
                g = g[:, :d]
            off = np.abs(g.reshape(r.shape) - r).max() / np.abs(r).max()
            print("%s net %d: %s gradient off by %.3g of its largest entry" % (what, k, name, off))
            assert off <= 1e-3, (k, name)
    _apply(S)
    tables = [(S["ents"][k], P["ents"][k], per[k][1], "ent %d" % k) for k in range(len(P["ents"]))] + [(S["attr"], P["attr"], g_attr, "attr")]
    for t, t0, g, name in tables:
        after = t.cpu().numpy()
        assert np.abs(after[:, d:]).max(initial=0.0) == 0.0
        got = t0 - after[:, :d].astype(np.float64)
        off = np.abs(got - g).max()
        bound = 1e-3 * np.abs(g).max() + U24 * np.abs(after).max()
        print("%s: %s gradient off by %.3g (bound %.3g, largest entry %.3g)" % (what, name, off, bound, np.abs(g).max()))
        assert off <= bound, name
        idle = np.abs(g).sum(1) == 0
        assert idle.any() and np.array_equal(after[idle, :d], t0[idle].astype(np.float32)), name
    assert int(sum(w.count_nonzero() for w in S["wss"])) == 0          # the apply phase left the scratch clean


@pytest.mark.parametrize("B,d", EDGE_SHAPES)
def test_cnn_gradients_at_edge_shapes(B, d):
    """two stacked nets (net 0 weighted), 7 attributes so that rows repeat, tables of 50 entities.  (3, 2): below one tile and a
    width below the kernel's; (33, 75): a batch tail with ld != d; (40, 100): the shipped d; (130, 128): the limit."""
    _check_grad_phase(ref.cnn_problem(1000 * d + B, B, d), "CNN B=%d d=%d" % (B, d))


def test_cnn_three_sgd_steps():
    """B = 5,000, d = 100, 2,000 entities, 400 attributes, two nets, three SGD steps (lr 0.01) with the engine's apply phase:
    tables through assert_rows_close (1e-4), parameters within 1e-4 of max |ref|."""
    from _tol import assert_rows_close
    from openea_amd import ops
    dev = ops.device()
    B, d, lr = 5000, 100, 0.01
    P = ref.cnn_problem(5, B, d, n_ent=2000, n_attr=400, n_lit=3000)
    rng = np.random.RandomState(6)
    S = _setup(P, dev, B, lr=lr)
    start = [e.copy() for e in P["ents"]]
    loss_ref = 0.0
    for _ in range(3):
        P["batch"] = np.stack([rng.randint(0, 1995, B), rng.randint(0, 399, B), rng.randint(0, 3000, B)], 1).astype(np.int32)
        loss_ref += ref.cnn_sgd_step(P, lr)
        _cnn(S, ops.to_ids(P["batch"], dev), ops.PHASE_BOTH)
        _apply(S)
    loss = float(S["loss"].item())
    print("three steps: loss %.9g (restatement %.9g, relative %.3g)" % (loss, loss_ref, abs(loss - loss_ref) / loss_ref))
    assert abs(loss - loss_ref) <= 2e-5 * loss_ref
    for k in range(2):
        assert_rows_close(S["ents"][k][:, :d].cpu().numpy(), P["ents"][k], "three steps: ent %d" % k)
        assert np.linalg.norm(P["ents"][k] - start[k]) > 0
        for name, t in zip(ref.VARS, S["params"][k]):
            r = P["params"][k][name]
            g = t.cpu().numpy().astype(np.float64)
            g = g[:, :d] if name == "W" else g
            off = np.abs(g.reshape(r.shape) - r).max() / np.abs(r).max()
            print("three steps: net %d %s off by %.3g of its largest entry" % (k, name, off))
            assert off <= 1e-4, (k, name)
    assert_rows_close(S["attr"][:, :d].cpu().numpy(), P["attr"], "three steps: attr")


def test_parameter_gradients_have_the_same_bits_run_to_run():
    """fixed-order fp64 sums: the eight gradients of both nets are bit-identical in two runs, in this build as in the other"""
    from openea_amd import ops
    dev = ops.device()
    P = ref.cnn_problem(77, 257, 100)
    runs = []
    for _ in range(2):
        S = _setup(P, dev, 300)
        _cnn(S, ops.to_ids(P["batch"], dev), ops.PHASE_GRAD)
        runs.append([g.clone() for k in range(2) for g in ops.multike_cnn_grads(S["ws"], k)] + [S["loss"].clone()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert float(runs[0][0].abs().sum()) > 0


DET_WORKER = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.environ["OEA_ROOT"]); sys.path.insert(0, os.path.join(os.environ["OEA_ROOT"], "tests"))
import torch
from openea_amd import ops
import _multike_ref as ref
from test_multike_gpu import _setup, _cnn, _apply, _variables
assert ops.deterministic()
dev = ops.device()
runs = []
for _ in range(2):
    P = ref.cnn_problem(9, 257, 100)
    S = _setup(P, dev, 257)
    start = [t.clone() for t in _variables(S)]
    for _ in range(2):
        _cnn(S, ops.to_ids(P["batch"], dev), ops.PHASE_BOTH)
        _apply(S)
    torch.cuda.synchronize()
    runs.append([t.cpu().numpy() for t in _variables(S)] + [S["loss"].cpu().numpy()])
moved = int(all(not np.array_equal(a, b.cpu().numpy()) for a, b in zip(runs[0][:3], start[:3])))
print("RESULT MultiKE same_bits=%d moved=%d" % (int(all(np.array_equal(a, b) for a, b in zip(*runs))), moved))
'''


def test_fixed_point_build_gives_the_same_bits():
    """libopenea_hip_det.so: two runs of two full steps (both nets, SGD on the parameters, the engine's apply phase) leave
    bit-identical tables, parameters and loss"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", DET_WORKER], env=dict(os.environ, OEA_ROOT=root, OEA_STEP_DETERMINISTIC="1"),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "RESULT MultiKE same_bits=1 moved=1" in p.stdout, p.stdout


@pytest.mark.parametrize("bad", ["dim", "ld", "n", "phase", "nets"])
def test_cnn_step_rejected_configurations_launch_nothing(bad):
    from openea_amd import ops
    from openea_amd._lib import OpenEAHipError
    dev = ops.device()
    P = ref.cnn_problem(3, 6, 8)
    S = _setup(P, dev, 6)
    batch = ops.to_ids(P["batch"], dev)
    before = [t.clone() for t in _variables(S)]
    with pytest.raises(OpenEAHipError):
        if bad == "dim":
            ops.multike_cnn_workspace(129, 132, 6, dev)
        elif bad == "ld":
            ops.multike_cnn_workspace(6, 6, 6, dev)
        elif bad == "n":
            _cnn(S, torch.cat([batch, batch]), ops.PHASE_GRAD)           # 12 > max_n
        elif bad == "phase":
            _cnn(S, batch, ops.PHASE_APPLY)
        else:
            S["nets"] = S["nets"][::-1]                                    # net 0's workspace does not hold the attribute rows
            _cnn(S, batch, ops.PHASE_GRAD)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(_variables(S), before))
    assert float(S["loss"].item()) == 0.0 and int(sum(w.count_nonzero() for w in S["wss"])) == 0


# ---- the row-wise terms ------------------------------------------------------------------------------------------------------------
N_ENT, N_REL = 200, 24            # the last 10 entities and the last 4 relations are in no item
N_SMALL = 3                       # items of the first launch: fewer than a workgroup has waves, on rows of their own


def _row_items(kind, n, rng, ent_lo, ent_hi, rel_lo, rel_hi):
    if kind in ("cross", "wsoft"):
        items = np.stack([rng.randint(ent_lo, ent_hi, n), rng.randint(rel_lo, rel_hi, n), rng.randint(ent_lo, ent_hi, n)], 1).astype(np.int32)
        items[0, 2] = items[0, 0]                                          # h == t
        items[2, 0] = items[1, 0]
    else:
        items = rng.randint(ent_lo, ent_hi, n).astype(np.int32)
        items[1] = items[0]                                                # an id twice in the batch counts twice
    return items


def _row_case(kind, d, n, rng):
    """Two launches into the same scratch, then one apply: N_SMALL items on entities [0, 6) and relation 0, then n items on the
    other rows.  The problem the gradients are held to is the sum of both, so E32 is taken over some hundred rows while the rows of
    the small launch check that launch alone.
    -> tables, (items of launch 1, of launch 2), weight, coef, restatement(dtype) -> (loss, [gA, gB, grel] w.r.t. the RAW rows;
    None where a table is constant)"""
    A, Bt, rel = (ref.f32(rng.standard_normal((rows, d)) / np.sqrt(d)) for rows in (N_ENT, N_ENT, N_REL))
    w = ref.f32(rng.randint(1, 65, N_REL) / 64.0)
    parts = (_row_items(kind, N_SMALL, rng, 0, 6, 0, 1), _row_items(kind, n, rng, 6, N_ENT - 10, 1, N_REL - 4))
    items = np.concatenate(parts)
    coef = {"cross": 1.0, "wsoft": 2.0, "pull": 0.5, "pull2": 1.0}[kind]

    def run(dt):
        a, b, r = A.astype(dt), Bt.astype(dt), rel.astype(dt)
        if kind == "cross":
            loss, ga, gb, gr = ref.cross_term(a, b, r, items, dt(coef))
        elif kind == "wsoft":
            loss, ga, gb, gr = ref.wsoft_term(a, b, r, items, w.astype(dt), dt(coef))
        else:
            loss, ga, gb = ref.pull_term(a, b, items, dt(coef))
            gr = None
            if kind == "pull":
                gb = None
        out = [ref.through_l2n(a, ga), None if gb is None else ref.through_l2n(b, gb), None if gr is None else ref.through_l2n(r, gr)]
        return loss, [None if g is None else g.astype(np.float64) for g in out]
    return (A, Bt, rel), parts, w, coef, run


ROW_CASES = [(kind, d, 128) for d in (2, 3, 64, 65, 75, 127, 128) for kind in ("cross", "wsoft", "pull", "pull2")] + \
            [("cross", 64, 8200), ("pull2", 64, 8200)]                    # past the grid cap of 2,048 workgroups of four waves


@pytest.mark.parametrize("kind,d,n", ROW_CASES)
def test_row_terms_one_sgd_step(kind, d, n):
    """one SGD step at lr = 1.0: before - after is the gradient (tests/_grads.py: gradient_check, 4 E32 + 2^-24 |after row| per row,
    E32 from the float32 run of the restatement); the loss within (d + 32) 2^-24 of the sum of its terms.  CROSS and WSOFT send the
    relation rows' gradient to the SECOND table's workspace, as the relation view does."""
    from _grads import gradient_check
    from openea_amd import ops
    dev = ops.device()
    rng = np.random.RandomState(100 * d + n + len(kind))
    tables, parts, w, coef, run = _row_case(kind, d, n, rng)
    loss64, g64 = run(np.float64)
    _, g32 = run(np.float32)
    A, Bt, rel = (ops.to_table(t, dev=dev) for t in tables)
    ld = A.shape[1]
    dummy = torch.zeros((1, ld), device=dev)
    ws_a, ws_b = ops.step_workspace(N_ENT, 1, ld, dev), ops.step_workspace(N_ENT, N_REL, ld, dev)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    code = {"cross": ops.MULTIKE_ROWS_CROSS, "wsoft": ops.MULTIKE_ROWS_WSOFT, "pull": ops.MULTIKE_ROWS_PULL, "pull2": ops.MULTIKE_ROWS_PULL}[kind]
    for items in parts:
        ops.multike_rows(code, A, ws_a, 1, Bt, None if kind == "pull" else ws_b, N_REL, None if kind.startswith("pull") else rel, d,
                         ops.to_ids(items, dev), coef, loss, rel_weight=ops.to_vec(w, dev), rel_side=1)
    cfg = ops.make_step_cfg(loss="positive", optimizer="SGD", lr=1.0, ent_l2_norm=True, rel_l2_norm=True)
    empty = torch.zeros((0, 3), dtype=torch.int32, device=dev)
    sink = torch.zeros(1, dtype=torch.float64, device=dev)
    ops.triple_step(A, None, dummy, None, d, empty, None, cfg, ws_a, sink, phase=ops.PHASE_APPLY)
    ops.triple_step(Bt, None, rel, None, d, empty, None, cfg, ws_b, sink, phase=ops.PHASE_APPLY)
    got = float(loss.item())
    bound = (d + 32) * U24 * abs(loss64)
    what = "%s d=%d n=%d" % (kind, d, n)
    print("%s: loss %.12g (float64 %.12g), off by %.3g (bound %.3g)" % (what, got, loss64, abs(got - loss64), bound))
    assert abs(got - loss64) <= bound
    for name, t, t0, a64, a32 in zip(("A", "B", "rel"), (A, Bt, rel), tables, g64, g32):
        after = t[:, :d].cpu().numpy()
        assert float(t[:, d:].abs().sum()) == 0.0
        if a64 is None:
            assert np.array_equal(after, t0.astype(np.float32)), name          # a constant table keeps its bits
            continue
        assert np.abs(a64[:6 if name != "rel" else 1]).max() > 0               # the small launch arrived
        gradient_check("%s %s" % (what, name), t0.astype(np.float32), after, a64, a32)
        idle = np.abs(a64).sum(1) == 0
        assert idle.any() and np.array_equal(after[idle], t0[idle].astype(np.float32)), name


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_end_to_end(tmp_path, capsys):
    """make_kgs("tiny", attributes=True, string_values=True) with synth.literal_vectors: eleven epochs with
    start_predicate_soft_alignment = 1, so that the predicate update at epoch 10 runs and epoch 11 trains on its result.  Every
    view's loss is finite, the relation view's loss falls, the 'nv' validation is ops.rank_eval on the name table, and the weight
    vectors on the device are add_weights' / generate_sup_predicate_triples' per-triple weights."""
    from openea_amd import ops
    from openea_amd.approaches import MultiKE
    from openea_amd.modules.base import initializers
    from openea_amd.modules.load import synth
    from openea_amd.run.default_args import get_args
    initializers.seed(20190719)
    d = 32
    kgs = synth.make_kgs("tiny", mode="swapping", seed=0, attributes=True, string_values=True)
    model = MultiKE()
    model.set_args(get_args("MultiKE", output=str(tmp_path) + "/out/", training_data="synthetic/tiny/", dataset_division="f/", dim=d,
                            batch_size=500, entity_batch_size=300, attribute_batch_size=400, max_epoch=11,
                            start_predicate_soft_alignment=1, learning_rate=0.005))
    model.set_kgs(kgs)
    model.literal_encoder = lambda literals: synth.literal_vectors(literals, d, 7)
    model.init()
    pm = model.predicate_align_model
    assert len(pm.attribute_id_alignment_set) > 0 and len(pm.relation_id_alignment_set) > 0
    start = [t.var.clone() for t in (model.ent_embeds, model.rv_ent_embeds, model.av_ent_embeds, model.attr_embeds, model.rel_embeds)]
    names0 = model.name_embeds.var.clone()
    model.run()
    model.test()
    out = capsys.readouterr().out
    print(out[-3000:])
    h = model.history
    for name in ("relation", "attribute", "common_space", "ckge_relation", "ckge_attribute", "ckgp_relation", "ckga_attribute"):
        assert len(h[name]) > 0 and all(np.isfinite(v) for v in h[name]), (name, h.get(name))
    assert len(h["relation"]) == 11 and len(h["attribute"]) == 11 and len(h["common_space"]) == 22
    assert len(h["ckgp_relation"]) == 10 and len(h["ckga_attribute"]) == 10          # from epoch 2 on
    assert h["relation"][9] < h["relation"][0]
    assert "update relation alignment:" in out and "update attribute alignment:" in out and "Training ends. Total time" in out
    # the name view never moves; its validation is rank_eval on its rows
    assert torch.equal(model.name_embeds.var, names0)
    dev = names0.device
    e1 = ops.gather_rows(names0, d, ops.to_ids(np.asarray(kgs.valid_entities1, np.int32), dev), normalize=True)
    e2 = ops.gather_rows(names0, d, ops.to_ids(np.asarray(kgs.valid_entities2 + kgs.test_entities2, np.int32), dev), normalize=True)
    rank, _ = ops.rank_eval(e1, e2, d, metric='inner')
    _, _, rr = ops.rank_metrics(rank, model.args.top_k)
    assert h["nv"][0] == rr / e1.shape[0]
    for t, t0 in zip((model.ent_embeds, model.rv_ent_embeds, model.av_ent_embeds, model.attr_embeds, model.rel_embeds), start):
        assert torch.isfinite(t.var).all() and not torch.equal(t.var, t0)
    # the weight vectors after the update against the per-triple weights of the host functions
    aw, saw, srw = (v.cpu().numpy() for v in (model._attr_w, model._sup_attr_w, model._sup_rel_w))
    for (_, p, _, w) in pm.attribute_triples_w_weights1 + pm.attribute_triples_w_weights2:
        assert aw[p] == np.float32(w)
    for (_, p, _, w) in pm.sup_attribute_alignment_triples1 + pm.sup_attribute_alignment_triples2:
        assert saw[p] == np.float32(w)
    for (_, p, _, w) in pm.sup_relation_alignment_triples1 + pm.sup_relation_alignment_triples2:
        assert srw[p] == np.float32(w)
    assert model._ckga_attr.shape[0] == len(pm.sup_attribute_alignment_triples1) + len(pm.sup_attribute_alignment_triples2) > 0


# ---- the reference's own graphs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["multike_d6", "multike_d16"])
def test_cnn_step_equals_reference_graphs(tag):
    """PHASE_GRAD on the fixture's batches (golden/multike_graph.npz: the reference's graphs under the TF stand-in, gradients by
    central differences): the attribute view (two nets on one batch, plus the pull towards the names through oea_multike_rows),
    then the two one-net cross-KG graphs.  Loss within 2e-5 relative, every gradient within 1e-3 of max |ref|, no variable moved;
    the tables' gradients through the engine's apply phase under SGD with lr = 1."""
    from test_multike_cpu import GOLDEN, fixture_case
    from openea_amd import ops
    dev = ops.device()
    z = np.load(GOLDEN)
    c = fixture_case(z, tag)
    d, t = c["d"], c["tables"]
    B = len(c["att"])
    aw = ops.to_vec(z[tag + "_attr_weight"], dev)
    assert np.array_equal(z[tag + "_attr_weight"][c["att"][:, 1]], c["att_w"])
    batch = ops.to_ids(c["att"], dev)
    lit, names = ops.to_table(c["lit"], dev=dev), ops.to_table(c["names"], dev=dev)
    E, A = t["ent_embeds"].shape[0], t["attr_embeds"].shape[0]
    graphs = [("attribute_loss", [(0, "av_ent_embeds", True, 1.0), (1, "ent_embeds", False, 1.0)]),
              ("ckge_attribute_loss", [(2, "av_ent_embeds", False, 2.0)]),
              ("ckga_attribute_loss", [(3, "av_ent_embeds", True, 1.0)])]
    for loss_name, nets_spec in graphs:
        attr = ops.to_table(t["attr_embeds"], dev=dev)
        ld = attr.shape[1]
        dummy = torch.zeros((1, ld), device=dev)
        ents, wss, nets, params = {}, {}, [], []
        for k, (i, table, weighted, factor) in enumerate(nets_spec):
            ents[table] = ops.to_table(t[table], dev=dev)
            wss[table] = ops.step_workspace(E, A if k == 0 else 1, ld, dev)
            params.append(_params_dev(c["sets"][i], d, dev))
            nets.append(ops.multike_net(params[-1], ents[table], wss[table], A if k == 0 else 1, weighted=weighted, factor=factor))
        ws = ops.multike_cnn_workspace(d, ld, B, dev)
        loss = torch.zeros(1, dtype=torch.float64, device=dev)
        everything = list(ents.values()) + [attr] + [p for ps in params for p in ps]
        before = [x.clone() for x in everything]
        ops.multike_cnn_step(nets, attr, lit, d, batch, aw, 1.0, ws, loss, phase=ops.PHASE_GRAD)
        if loss_name == "attribute_loss":
            ops.multike_rows(ops.MULTIKE_ROWS_PULL, ents["ent_embeds"], wss["ent_embeds"], 1, names, None, 1, None, d,
                             batch[:, 0].contiguous(), 0.5, loss, b_l2_norm=False)
        got, want = float(loss.item()), float(z["%s_%s" % (tag, loss_name)][0])
        print("%s %s: loss %.9g (fixture %.9g, relative %.3g)" % (tag, loss_name, got, want, abs(got - want) / want))
        assert abs(got - want) <= 2e-5 * want
        assert all(torch.equal(a, b) for a, b in zip(everything, before))
        for k, (i, table, _, _) in enumerate(nets_spec):
            for name, g in zip(ref.VARS, ops.multike_cnn_grads(ws, k)):
                r = z["%s_%s_grad_cnn%d_%s" % (tag, loss_name, i, name)]
                g = g.cpu().numpy().astype(np.float64)
                g = g[:, :d] if name == "W" else g
                off = np.abs(g.reshape(r.shape) - r).max() / np.abs(r).max()
                print("%s %s: cnn%d %s gradient off by %.3g of its largest entry" % (tag, loss_name, i, name, off))
                assert off <= 1e-3, (loss_name, i, name)
        cfg = ops.make_step_cfg(loss="positive", optimizer="SGD", lr=1.0, ent_l2_norm=True, rel_l2_norm=False)
        empty = torch.zeros((0, 3), dtype=torch.int32, device=dev)
        sink = torch.zeros(1, dtype=torch.float64, device=dev)
        for k, (_, table, _, _) in enumerate(nets_spec):
            ops.triple_step(ents[table], None, attr if k == 0 else dummy, None, d, empty, None, cfg, wss[table], sink, phase=ops.PHASE_APPLY)
        for table, dev_t in list(ents.items()) + [("attr_embeds", attr)]:
            r = z["%s_%s_grad_%s" % (tag, loss_name, table)]
            after = dev_t[:, :d].cpu().numpy()
            off = np.abs((t[table] - after.astype(np.float64)) - r).max()
            bound = 1e-3 * np.abs(r).max() + U24 * np.abs(after).max()
            print("%s %s: %s gradient off by %.3g (bound %.3g)" % (tag, loss_name, table, off, bound))
            assert off <= bound, (loss_name, table)
