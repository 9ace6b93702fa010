"""The fused steps that launch a capped grid and walk their batch in a grid-stride loop -- hole_kernel, simple_kernel,
distmult_kernel (csrc/semantic_step.hip), jape_kernel (csrc/jape_step.hip), weighted_pair_kernel and path_convert_kernel
(csrc/ptranse_step.hip), mapping_links_kernel (csrc/mapping.hip), rotate_triples (csrc/rotate_step.hip) -- past their caps, and
the fp32 ones held to float64 GRADIENTS per row at the dimensions where a lane pair, the doubled LDS operand of HolE or the
register slots of row_ops.h can go wrong.  tests/_grads.py has the problems, the references and the two tolerances: one SGD step
with lr = 1.0, before - after against the float64 gradient within 4 E32 + 2^-24 |after row|; the loss within
(d + 32) 2^-24 sum |term|.  Every test prints deviation / (4 E32) and measured / bound."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import _grads as G  # noqa: E402
from test_iptranse_gpu import _align_step as _pair_step, _setup as _pair_setup  # noqa: E402
from test_jape_gpu import _setup as _jape_setup, _step as _jape_step  # noqa: E402
from test_rotate_distmult_cpu import _rotate_batch, rotate_reference_step  # noqa: E402
from test_rotate_distmult_gpu import _assert_rotate_close, _dm_setup, _dm_step, _rotate_setup, _rotate_steps  # noqa: E402
from test_semantic_gpu import _setup as _sem_setup, _step as _sem_step  # noqa: E402

K_MODELS = ("HolE", "SimplE", "DistMult", "JAPE")          # k negatives per positive; the weighted pairs have one


def _device_step(p, dev, optimizer="SGD"):
    """one step with lr = 1.0 -> the state dict of the model's own test module (e, r: the device tables)"""
    from openea_amd import ops
    model, tables, b = p["model"], p["tables"], p["batch"]
    pos, neg = ops.to_ids(b["pos"], dev), ops.to_ids(b["neg"], dev)
    if model in ("HolE", "SimplE"):
        s = _sem_setup(model, tables, optimizer, dev, k=b["k"], margin=b["margin"], lr=1.0)
        _sem_step(s, pos, neg)
    elif model == "DistMult":
        s = _dm_setup(tables, optimizer, dev, k=b["k"], lr=1.0)
        _dm_step(s, pos, neg)
    elif model == "JAPE":
        s = _jape_setup(tables, optimizer, dev, b["k"], 1.0)
        _jape_step(s, pos, neg, neg_alpha=b["neg_alpha"])
    else:
        s = _pair_setup(tables, optimizer, dev, lr=1.0, margin=b["margin"])
        _pair_step(s, b)
    torch.cuda.synchronize()
    return s


def _split(model, e, r):
    """device tables -> host arrays in the order of the restatement's tables (SimplE: [H; T], [R1; R2] unstacked)"""
    e, r = e.cpu().numpy(), r.cpu().numpy()
    if model != "SimplE":
        return [e, r]
    return [e[:G.N_ENT], e[G.N_ENT:], r[:G.N_REL], r[G.N_REL:]]


def _named(p, n_rows, is_rel):
    b = p["batch"]
    cols = [1] if is_rel else [0, 2]
    ids = np.concatenate([b["pos"][:, cols].reshape(-1), b["neg"][:, cols].reshape(-1)])
    mask = np.zeros(n_rows, bool)
    mask[ids] = True
    return mask


def _check(p, s, what, loss=True):
    """gradients per row, the loss, rows no triple names, the pad columns, the workspace -> (worst gradient ratio, loss ratio)"""
    model, d = p["model"], p["dim"]
    after = _split(model, s["e"], s["r"])
    ratios = []
    for i, (t0, a, g64, g32) in enumerate(zip(p["tables"], after, p["g64"], p["g32"])):
        is_rel = t0.shape[0] == G.N_REL
        before = t0.astype(np.float32)
        assert not a[:, d:].any(), "%s table %d: pad columns" % (what, i)
        floor = G.one_column_floor(p, i) if d == 1 else 0.0
        ratios.append(G.gradient_check("%s table %d" % (what, i), before, np.ascontiguousarray(a[:, :d]), g64, g32, floor))
        named = _named(p, t0.shape[0], is_rel)
        assert not named[-(G.REL_TAIL if is_rel else G.ENT_TAIL):].any()
        assert np.array_equal(a[~named, :d], before[~named]), "%s table %d: a row no triple names moved" % (what, i)
    assert int(s["ws"][: -8 * 4096].count_nonzero()) == 0, what + ": the step workspace is not clean"
    loss_ratio = G.loss_check(what, float(s["loss"].item()), p, d) if loss else 0.0
    return max(ratios), loss_ratio


def _case(model, dim, n_pos, k, margin=0.2):
    from openea_amd import ops
    dev = ops.device()
    p = G.problem(model, dim, n_pos, 1 if model == "WPair" else k, margin)
    s = _device_step(p, dev)
    what = "%s d=%d n=%d k=%d" % (model, dim, n_pos, p["batch"]["k"])
    if "active" in p["batch"]:
        what += " (%.0f%% active, %d left out)" % (100 * p["batch"]["active"], p["batch"]["dropped"])
    return _check(p, s, what)


# ---- 1. dimensions: ld > dim with d odd, the last lane with one real column, the lane + 64 half of flush_row empty / half / full
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("dim", [1, 2, 3, 64, 65, 75, 127, 128])
@pytest.mark.parametrize("model", K_MODELS)
def test_gradients_at_edge_dimensions(model, dim, k):
    _case(model, dim, 37, k)


@pytest.mark.parametrize("dim", [1, 2, 3, 64, 65, 75, 127, 128])
def test_pair_gradients_at_edge_dimensions(dim):
    _case("WPair", dim, 37, 1)


# ---- 2. fewer waves than a block: its last waves skip the loop and go straight to the barrier
@pytest.mark.parametrize("n_pos", [1, 3, 5])
@pytest.mark.parametrize("model", G.MODELS)
def test_gradients_below_one_block(model, n_pos):
    _case(model, 75, n_pos, 3)


# ---- 3. past the cap of 2,048 blocks x 4 waves = 8,192 positives: the second and the third trip of the grid-stride loop
@pytest.mark.parametrize("n_pos", [8195, 16389])
@pytest.mark.parametrize("dim", [6, 128])
@pytest.mark.parametrize("model", G.MODELS)
def test_gradients_past_the_grid_cap(model, dim, n_pos):
    """8,195: the second trip is taken by three waves of block 0 alone; 16,389: a third trip.  A skipped or doubled trip shows
    in the loss as well as in the gradients (the loss is asserted in every test of this file)."""
    assert n_pos > 2048 * 4
    _case(model, dim, n_pos, 3 if model in ("DistMult", "JAPE") else 1)


# ---- 4. HolE's hinge
@pytest.mark.parametrize("k", [1, 3])
def test_hole_every_hinge_active(k):
    """margin 2.0: the sigmoids lie in (0, 1), no positive is skipped"""
    _case("HolE", 75, 37, k, margin=2.0)


@pytest.mark.parametrize("k", [2, 3])
def test_hole_mixed_hinges(k):
    """margin 0.0 with random rows: between a quarter and three quarters of the hinges are active (asserted where the problem
    is built); 203 positives so that up to two may lie on the kink and be left out.  (k = 1 would put the batch's negative that
    is identical to its positive on the kink, l = 0.0: test_hole_zero_hinges_change_nothing has that case.)"""
    _case("HolE", 75, 203, k, margin=0.0)


@pytest.mark.parametrize("k", [1, 2])
def test_hole_zero_hinges_change_nothing(k):
    """margin 0.0 and every negative identical to its positive: l = -s + (s + ... + s) / k is 0.0 exactly for k = 1, 2 (k = 3
    is left out on purpose: 3 s fl(1 / 3) need not equal s).  Loss 0.0, tables and accumulators keep their bits, nothing is
    flagged."""
    from openea_amd import ops
    dev = ops.device()
    p = G.problem("HolE", 75, 37, k, 0.0, True)
    assert p["loss64"] == 0.0 and all(not g.any() for g in p["g64"])
    s = _device_step(p, dev, "Adagrad")
    assert float(s["loss"].item()) == 0.0
    for t0, t in zip(p["tables"], (s["e"], s["r"])):
        assert torch.equal(t, ops.to_table(t0, dev=dev))
    for a in s["accs"]:
        assert torch.equal(a, torch.full_like(a, 0.1))
    assert int(s["ws"][: -8 * 4096].count_nonzero()) == 0


# ---- 5. MTransE's mapping step: 1,024 x 4 = 4,096 links (M in LDS, d <= 120), 4,096 x 4 = 16,384 links (M in global memory)
@pytest.mark.parametrize("d,n", [(8, 4099), (100, 4099), (130, 16387), (100, 1), (130, 1)])
def test_mapping_gradients_past_the_grid_cap(d, n):
    """loss, M and the entity rows (after the apply phase) against the SGD restatement of test_mapping_step_matches_oracle"""
    from openea_amd import ops
    dev = ops.device()
    p = G.mapping_problem(d, n)
    n_ent = p["ent"].shape[0]
    te = ops.to_table(p["ent"], dev=dev)
    tm = torch.from_numpy(p["M"].astype(np.float32)).to(dev).contiguous()
    rel = ops.to_table(np.ones((3, d)), dev=dev)
    cfg = ops.make_step_cfg(loss="positive", optimizer="SGD", lr=1.0)
    ws = ops.step_workspace(n_ent, 3, te.shape[1], dev)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    dummy = torch.zeros(1, dtype=torch.float64, device=dev)
    empty = torch.zeros((0, 3), dtype=torch.int32, device=dev)
    ids1, ids2 = ops.to_ids(p["links"][:, 0].copy(), dev), ops.to_ids(p["links"][:, 1].copy(), dev)
    ops.mapping_step(te, d, True, ids1, ids2, tm, None, p["alpha"], 1.0, "SGD", ws, n_ent, 3, loss, None)
    ops.triple_step(te, None, rel, None, d, empty, None, cfg, ws, dummy, phase=ops.PHASE_APPLY)
    torch.cuda.synchronize()
    what = "mapping d=%d n=%d" % (d, n)
    e = te.cpu().numpy()
    assert not e[:, d:].any()
    G.gradient_check(what + " entity rows", p["ent"].astype(np.float32), np.ascontiguousarray(e[:, :d]), p["g64"][0], p["g32"][0])
    G.gradient_check(what + " M", p["M"].astype(np.float32), tm.cpu().numpy(), p["g64"][1], p["g32"][1])
    named = np.zeros(n_ent, bool)
    named[p["links"].reshape(-1)] = True
    assert not named[-100:].any() and np.array_equal(e[~named, :d], p["ent"].astype(np.float32)[~named])
    assert float(dummy.item()) == 0.0
    assert int(ws[: -8 * 4096].count_nonzero()) == 0
    G.loss_check(what, float(loss.item()), p, d)


# ---- 6. RotatE: 4,096 blocks x 8 groups = 32,768 items at ld <= 128
@pytest.mark.parametrize("k", [17, 0])
def test_rotate_past_the_grid_cap(k):
    """d = 8.  k = 17: two chunks per family, 16,387 families = 32,774 items.  k = 0 (free negatives): 16,387 positives and as
    many negatives, one item each.  Tables and state are fp64: the tolerances of test_rotate_weighted_negatives_equal_restatement."""
    from openea_amd import ops
    dev = ops.device()
    d, n_pos, E, R = 8, 16387, 400, 9
    rng = np.random.RandomState(2000 + k)
    ent = rng.standard_normal((2 * E, d)) / np.sqrt(d)
    rel = rng.standard_normal((R, d)) / np.sqrt(d)
    pos, neg = _rotate_batch(rng, E, R, n_pos, max(k, 1))
    items = n_pos * 2 if k else n_pos + len(neg)
    assert items > 4096 * (256 // 32)
    div = k if k else 1
    kw = dict(gamma=6.0, ent_l2_norm=True, rel_l2_norm=True, optimizer="Adam", lr=0.01)
    e_ref, r_ref, st = ent.copy(), rel.copy(), {}
    ref_loss = sum(rotate_reference_step(e_ref, r_ref, pos, neg, st, phase_scale=np.pi / (8.0 / d), neg_loss_div=div, **kw)
                   for _ in range(2))
    s = _rotate_setup(ent, rel, d, dev, dim=d, neg_loss_div=div, **kw)
    _rotate_steps(s, ops.to_ids(pos, dev), ops.to_ids(neg, dev), k, 2)
    _assert_rotate_close(s, d, ref_loss, e_ref, r_ref, "RotatE d=%d k=%d, %d items" % (d, k, items))


# ---- 7. IPTransE's path half in the fixed-point build: path_convert_kernel walks A^T with at most 1,024 x 256 threads
PATH_R, PATH_D, PATH_N = 520, 16, 3000
PATH_WORKER = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.environ["OEA_ROOT"]); sys.path.insert(0, os.path.join(os.environ["OEA_ROOT"], "tests"))
import torch
import _grads as G
from openea_amd import ops
from test_iptranse_gpu import _dev_batch, _setup
from test_step_edges_gpu import PATH_D, PATH_N, PATH_R
assert ops.deterministic()
dev = ops.device()
p = G.path_problem(PATH_R, PATH_D, PATH_N)
s = _setup(p["tables"], "SGD", dev, lr=1.0, margin=p["batch"]["margin"])
d = _dev_batch(p["batch"], dev)
ops.path_grad(s["r"], PATH_D, d["paths"], d["neg_rel"], d["weight"], p["batch"]["margin"], p["batch"]["path_parm"], True, s["ws"],
              p["tables"][0].shape[0], s["pws"], s["loss"])
ops.triple_step(s["e"], None, s["r"], None, PATH_D, d["pos"], None, s["cfg"], s["ws"], s["loss"], phase=ops.PHASE_APPLY)
torch.cuda.synchronize()
np.savez(os.environ["OEA_OUT"], rel=s["r"].cpu().numpy(), ent=s["e"].cpu().numpy(), loss=s["loss"].cpu().numpy(),
         ws=np.array([int(s["ws"][: -8 * 4096].count_nonzero())]))
print("RESULT done")
'''


def test_path_half_past_the_convert_cap(tmp_path):
    """oea_path_grad refuses n_rel > 2,048, so Rp^2 reaches 4 M entries: the cap of 262,144 threads is below that from n_rel = 513
    on.  path_convert_kernel exists in libopenea_hip_det.so only (OEA_STEP_DETERMINISTIC=1), hence the child process.  n_rel = 520:
    270,400 entries of A^T, the columns of relations 505 and up lie past the first trip and the batch names them."""
    import subprocess
    import sys
    p = G.path_problem(PATH_R, PATH_D, PATH_N)
    b = p["batch"]
    assert PATH_R * PATH_R > 1024 * 256 and PATH_R % 4 == 0
    cols = np.concatenate([b["paths"].reshape(-1), b["neg_rel"]])
    assert (cols.astype(np.int64) * PATH_R > 1024 * 256).sum() > 50 and 0.2 < b["active"] < 1.0
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "path.npz")
    run = subprocess.run([sys.executable, "-c", PATH_WORKER], env=dict(os.environ, OEA_ROOT=root, OEA_STEP_DETERMINISTIC="1", OEA_OUT=out),
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "RESULT done" in run.stdout, run.stderr[-2000:]
    z = np.load(out)
    what = "path half R=%d d=%d n=%d (%.0f%% active, %d left out)" % (PATH_R, PATH_D, PATH_N, 100 * b["active"], b["dropped"])
    G.gradient_check(what + " relation table", p["tables"][1].astype(np.float32), np.ascontiguousarray(z["rel"][:, :PATH_D]), p["g64"],
                     p["g32"])
    assert np.array_equal(z["ent"][:, :PATH_D], p["tables"][0].astype(np.float32))
    assert np.array_equal(z["rel"][-G.REL_TAIL:, :PATH_D], p["tables"][1].astype(np.float32)[-G.REL_TAIL:])
    assert int(z["ws"][0]) == 0
    G.loss_check(what, float(z["loss"][0]), p, PATH_D)
