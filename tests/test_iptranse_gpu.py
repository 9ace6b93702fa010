"""IPTransE on the device (csrc/ptranse_step.hip: oea_path_grad, oea_ptranse_step, oea_path_sample_epoch, oea_ptranse_epoch,
oea_weighted_pair_step): against the reference's own graphs (tests/golden/iptranse_graph.npz), against the float64 restatement
of test_iptranse_cpu.py -- which gathers rows, where the device goes through the Gram matrix --, the path half alone, the epoch
call against the step loop, the path sampler, the configurations the steps refuse, and end to end through the IPTransE class."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_iptranse_cpu import CASES, GOLDEN, fixture_case, iptranse_reference_step  # noqa: E402

MARGIN, PATH_PARM = 1.5, 0.1
# A pair whose float64 hinge argument lies within 1e-5 of zero could flip in fp32 (the Gram form's error is a few 1e-7 on O(1)
# terms).  The problems below are drawn with the first seed (found on the CPU) for which the float64 reference has NO such pair,
# triple or path, in any of the three steps; the tests assert that condition again.
KINK = 1e-5
SEEDS = {8: 0, 75: 0, 100: 0, 128: 0, "small": 0, "path_only": 0}


def _setup(tables, optimizer, dev, lr=0.01, margin=MARGIN, loss_norm="L2", l2n=(True, True)):
    from openea_amd import ops
    e, r = ops.to_table(tables[0], dev=dev), ops.to_table(tables[1], dev=dev)
    dense = optimizer in ("Adam", "Adadelta")
    if dense:
        accs = [torch.zeros((2,) + tuple(t.shape), device=dev) for t in (e, r)]
    elif optimizer == "Adagrad":
        accs = [torch.full_like(e, 0.1), torch.full_like(r, 0.1)]
    else:
        accs = [None, None]
    cfg = ops.make_step_cfg(loss="margin-based", loss_norm=loss_norm, margin=margin, optimizer=optimizer, lr=lr,
                            ent_l2_norm=l2n[0], rel_l2_norm=l2n[1])
    cfg.opt_t = 1
    return dict(e=e, r=r, d=np.asarray(tables[0]).shape[1], accs=accs, cfg=cfg, ws=ops.step_workspace(e.shape[0], r.shape[0], e.shape[1], dev),
                pws=ops.path_workspace(r.shape[0], r.shape[1], dev), loss=torch.zeros(1, dtype=torch.float64, device=dev), dev=dev)


def _dev_batch(batch, dev):
    from openea_amd import ops
    out = dict(pos=ops.to_ids(np.asarray(batch["pos"], np.int32).reshape(-1, 3), dev),
               neg=ops.to_ids(np.asarray(batch["neg"], np.int32).reshape(-1, 3), dev))
    if "paths" in batch:
        out.update(paths=ops.to_ids(np.asarray(batch["paths"], np.int32).reshape(-1, 3), dev),
                   neg_rel=ops.to_ids(np.asarray(batch["neg_rel"], np.int32), dev), weight=ops.to_vec(batch["weight"], dev))
    else:
        out["weight"] = ops.to_vec(batch["weight"], dev)
    return out


def _train_step(s, batch, path_parm=PATH_PARM):
    from openea_amd import ops
    b = _dev_batch(batch, s["dev"])
    ops.ptranse_step(s["e"], s["accs"][0], s["r"], s["accs"][1], s["d"], b["pos"], b["neg"], b["paths"], b["neg_rel"], b["weight"],
                     path_parm, s["cfg"], s["ws"], s["pws"], s["loss"])


def _align_step(s, batch):
    from openea_amd import ops
    b = _dev_batch(batch, s["dev"])
    ops.weighted_pair_step(s["e"], s["accs"][0], s["r"], s["accs"][1], s["d"], b["pos"], b["neg"], b["weight"], s["cfg"], s["ws"],
                           s["loss"])


def _host(s):
    d = s["d"]
    return [s["e"][:, :d].cpu().numpy().astype(np.float64), s["r"][:, :d].cpu().numpy().astype(np.float64)]


@pytest.mark.parametrize("which", ["train", "align"])
@pytest.mark.parametrize("case", CASES)
def test_sgd_step_equals_reference_graph(case, which):
    from openea_amd import ops
    dev = ops.device()
    z = np.load(GOLDEN)
    tables, train, align = fixture_case(z, case)
    lr = 0.01
    s = _setup(tables, "SGD", dev, lr=lr, margin=train["margin"])
    if which == "train":
        _train_step(s, train, train["path_parm"])
    else:
        _align_step(s, align)
    loss, ref_loss = float(s["loss"].item()), float(z["%s_%s_loss" % (case, which)][0])
    print("%s %s: loss %.9g, reference %.9g, relative %.3g" % (case, which, loss, ref_loss, abs(loss - ref_loss) / abs(ref_loss)))
    assert abs(loss - ref_loss) <= 2e-5 * abs(ref_loss)
    for name, before, got in zip(("ent_embeds", "rel_embeds"), tables, _host(s)):
        g = (before.astype(np.float32).astype(np.float64) - got) / lr          # SGD: the update IS lr * gradient
        ref = z["%s_%s_grad_%s" % (case, which, name)]
        print("%s %s %s: gradient deviation %.3g of max %.3g" % (case, which, name, np.abs(g - ref).max(), np.abs(ref).max()))
        assert np.abs(g - ref).max() <= 1e-3 * np.abs(ref).max(), name
    d = s["d"]
    assert not s["e"][:, d:].any() and not s["r"][:, d:].any()                 # padding columns stay zero


def _xavier(rng, rows, dim):
    from openea_amd.modules.base.initializers import xavier_host
    return xavier_host(rng, (rows, dim)).astype(np.float32).astype(np.float64)


def _zipf_rel(rng, common, n):
    p = 1.0 / np.arange(1, common + 1) ** 1.1
    return rng.choice(common, n, p=p / p.sum())


def _path_batch(rng, n_rel, n, lone=True):
    """n path pairs with Zipf(1.1) relations over the first n_rel - 4 (a handful of A's entries take thousands of adds); r' == r
    in the first 40, r_x == r_y in the next 40, and -- lone -- the rarest of those relations in exactly one path"""
    common = n_rel - 4 if n_rel > 8 else n_rel
    q = np.stack([_zipf_rel(rng, common, n) for _ in range(4)], 1).astype(np.int32)
    k = min(40, n // 4)
    q[:k, 3] = q[:k, 2]
    q[k:2 * k, 1] = q[k:2 * k, 0]
    if lone:
        q[q == common - 1] = common - 2
        q[2 * k, 2] = common - 1
    w = rng.randint(1, 101, n).astype(np.float64)
    return dict(paths=q[:, :3], neg_rel=q[:, 3], weight=w)


def _problem(dim, n_ent, n_rel, n_tri, n_path, seed, steps=3):
    """-> tables [ent, rel] (float32-representable float64) and `steps` batches"""
    from test_semantic_gpu import _zipf_batch
    rng = np.random.RandomState(seed)
    tables = [_xavier(rng, n_ent, dim), _xavier(rng, n_rel, dim)]
    batches = []
    for _ in range(steps):
        if n_tri == 0:
            pos = neg = np.zeros((0, 3), np.int32)
        elif n_rel > 8:
            pos, neg = _zipf_batch(rng, n_ent, n_rel, n_tri)
        else:
            pos = np.stack([rng.randint(0, n_ent, n_tri), rng.randint(0, n_rel, n_tri), rng.randint(0, n_ent, n_tri)], 1).astype(np.int32)
            neg = pos.copy()
            neg[:, 2] = rng.randint(0, n_ent, n_tri)
        b = _path_batch(rng, n_rel, n_path, lone=n_rel > 8)
        b.update(pos=pos, neg=neg, margin=MARGIN, path_parm=PATH_PARM)
        batches.append(b)
    return tables, batches


def _adagrad_case(dim, n_ent, n_rel, n_tri, n_path, seed):
    from _tol import assert_rows_close
    from openea_amd import ops
    dev = ops.device()
    tables, batches = _problem(dim, n_ent, n_rel, n_tri, n_path, seed)
    s = _setup(tables, "Adagrad", dev)
    ref, accs = [t.copy() for t in tables], [np.full_like(t, 0.1) for t in tables]
    loss_ref, nearest = 0.0, np.inf
    for b in batches:
        l, _, near = iptranse_reference_step(ref, accs, b, 0.01, "Adagrad")
        loss_ref += l
        nearest = min(nearest, near)
        _train_step(s, b)
    assert nearest > KINK, "the float64 reference has a hinge argument within %g of zero (%g): choose another seed" % (KINK, nearest)
    loss = float(s["loss"].item())
    print("d=%d R=%d: loss %.9g, reference %.9g, relative %.3g; nearest hinge argument %.3g"
          % (dim, n_rel, loss, loss_ref, abs(loss - loss_ref) / abs(loss_ref), nearest))
    assert abs(loss - loss_ref) <= 2e-5 * abs(loss_ref)
    got = _host(s)
    got_acc = [a[:, :dim].cpu().numpy().astype(np.float64) for a in s["accs"]]
    for i, (g, r) in enumerate(zip(got, ref)):
        assert_rows_close(g, r, "IPTransE d=%d R=%d table %d" % (dim, n_rel, i))
    for i, (g, r) in enumerate(zip(got_acc, accs)):
        assert_rows_close(g, r, "IPTransE d=%d R=%d accumulator %d" % (dim, n_rel, i))
    assert not s["e"][:, dim:].any() and not s["r"][:, dim:].any()
    return tables, batches, got, got_acc


@pytest.mark.parametrize("dim", [8, 75, 100, 128])
def test_adagrad_steps_equal_restatement(dim):
    """three Adagrad steps, 2,000 triple pairs + 4,999 path pairs, n_rel = 477 (A and G padded to 480); dim = 75 has ld != dim.
    Relation rows nothing refers to keep their bits and their accumulators stay at 0.1."""
    n_rel = 477
    tables, batches, got, got_acc = _adagrad_case(dim, 3000, n_rel, 2000, 4999, SEEDS[dim])
    for b in batches:
        q = np.concatenate([b["paths"].reshape(-1), b["neg_rel"]])
        assert q.max() < n_rel - 4 and max(b["pos"][:, 1].max(), b["neg"][:, 1].max()) < n_rel - 4
        assert (b["paths"] == n_rel - 5).sum() + (b["neg_rel"] == n_rel - 5).sum() == 1          # in exactly one path
        assert (b["paths"][:, 2] == b["neg_rel"]).sum() >= 40 and (b["paths"][:, 0] == b["paths"][:, 1]).sum() >= 40
        assert np.bincount(q).max() > 1000                                                     # a hot entry of A
    assert np.array_equal(got[1][-4:], tables[1][-4:]) and (got_acc[1][-4:] == np.float32(0.1)).all()
    assert not np.array_equal(got[1][:-4], tables[1][:-4])
    assert np.array_equal(got[0][-100:], tables[0][-100:]) and (got_acc[0][-100:] == np.float32(0.1)).all()


def test_adagrad_steps_below_one_tile():
    """n_rel = 5 (padded to 8: far below one tile of the products), 37 path pairs"""
    _adagrad_case(16, 50, 5, 20, 37, SEEDS["small"])


def _path_only_problem(seed=None):
    tables, batches = _problem(100, 300, 477, 0, 4999, SEEDS["path_only"] if seed is None else seed, steps=1)
    b = batches[0]
    b["pos"], b["neg"] = np.zeros((0, 3), np.int32), np.zeros((0, 3), np.int32)
    return tables, b


def test_path_half_alone():
    """n_pos == 0, SGD: the relation table moves as in the restatement, the entity table keeps its bits"""
    from _tol import assert_rows_close
    from openea_amd import ops
    dev = ops.device()
    tables, b = _path_only_problem()
    s = _setup(tables, "SGD", dev)
    e0 = s["e"].clone()
    ref = [t.copy() for t in tables]
    loss_ref, _, nearest = iptranse_reference_step(ref, [None, None], b, 0.01, "SGD")
    assert nearest > KINK
    _train_step(s, b)
    loss = float(s["loss"].item())
    assert abs(loss - loss_ref) <= 2e-5 * abs(loss_ref)
    assert_rows_close(_host(s)[1], ref[1], "path half alone, relation table")
    assert torch.equal(s["e"], e0)
    assert not torch.equal(s["r"], ops.to_table(tables[1], dev=dev))
    # the same gradient through oea_path_grad + the apply phase
    s2 = _setup(tables, "SGD", dev)
    d = _dev_batch(b, dev)
    ops.path_grad(s2["r"], 100, d["paths"], d["neg_rel"], d["weight"], MARGIN, PATH_PARM, True, s2["ws"], 300, s2["pws"], s2["loss"])
    ops.triple_step(s2["e"], None, s2["r"], None, 100, d["pos"], None, s2["cfg"], s2["ws"], s2["loss"], phase=ops.PHASE_APPLY)
    assert_rows_close(_host(s2)[1], ref[1], "oea_path_grad + apply, relation table")


def _epoch_problem(dev, P_on=True, seed=5):
    """3 steps: tables, positives / negatives back to back with their offsets, path lists of 966 + 544 paths"""
    from openea_amd import ops
    from test_semantic_gpu import _zipf_batch
    rng = np.random.RandomState(seed)
    n_ent, n_rel, dim = 3000, 477, 100
    tables = [_xavier(rng, n_ent, dim), _xavier(rng, n_rel, dim)]
    sizes = [700, 700, 413]
    pn = [_zipf_batch(rng, n_ent, n_rel, n) for n in sizes]
    pos_all = ops.to_ids(np.concatenate([p for p, _ in pn]), dev)
    neg_all = ops.to_ids(np.concatenate([n for _, n in pn]), dev)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    sampled = None
    if P_on:
        lists = []
        for n, lo, hi in ((966, 0, 267), (544, 267, 473)):
            q = rng.randint(lo, hi, (n, 3)).astype(np.int32)
            lists += [ops.to_ids(q, dev), ops.to_vec(rng.randint(1, 101, n).astype(np.float32), dev),
                      ops.to_ids(np.arange(lo, hi, dtype=np.int32), dev)]
        sampled = ops.path_sample_epoch(lists[0], lists[1], lists[3], lists[4], lists[2], lists[5], 3, seed=11, epoch=4)
        assert sampled[0].shape == (3, 503, 3)
    return tables, pos_all, neg_all, offsets, sampled


def _run_epoch_and_loop(dev):
    from openea_amd import ops
    tables, pos_all, neg_all, offsets, sampled = _epoch_problem(dev)
    a, b = _setup(tables, "Adagrad", dev), _setup(tables, "Adagrad", dev)
    ops.ptranse_epoch(a["e"], a["accs"][0], a["r"], a["accs"][1], 100, pos_all, offsets, neg_all, sampled, PATH_PARM, a["cfg"], a["ws"],
                      a["pws"], a["loss"])
    for s in range(3):
        lo, hi = int(offsets[s]), int(offsets[s + 1])
        ops.ptranse_step(b["e"], b["accs"][0], b["r"], b["accs"][1], 100, pos_all[lo:hi], neg_all[lo:hi], sampled[0][s], sampled[1][s],
                         sampled[2][s], PATH_PARM, b["cfg"], b["ws"], b["pws"], b["loss"])
    torch.cuda.synchronize()
    return tables, a, b


def test_epoch_call_equals_the_step_loop():
    from _tol import assert_rows_close
    from openea_amd import ops
    dev = ops.device()
    tables, a, b = _run_epoch_and_loop(dev)
    for i, (x, y) in enumerate(zip(_host(a), _host(b))):
        assert_rows_close(x, y, "epoch call against step loop, table %d" % i)
        assert not np.array_equal(x, tables[i].astype(np.float32).astype(np.float64))
    la, lb = float(a["loss"].item()), float(b["loss"].item())
    assert abs(la - lb) <= 1e-5 * abs(lb) and la > 0


def test_epoch_call_without_paths_is_the_margin_step():
    """P = 0: the tables are row-close to ops.triple_step on the same batches"""
    from _tol import assert_rows_close
    from openea_amd import ops
    dev = ops.device()
    tables, pos_all, neg_all, offsets, _ = _epoch_problem(dev, P_on=False)
    a, b = _setup(tables, "Adagrad", dev), _setup(tables, "Adagrad", dev)
    ops.ptranse_epoch(a["e"], a["accs"][0], a["r"], a["accs"][1], 100, pos_all, offsets, neg_all, None, PATH_PARM, a["cfg"], a["ws"],
                      a["pws"], a["loss"])
    for s in range(3):
        lo, hi = int(offsets[s]), int(offsets[s + 1])
        ops.triple_step(b["e"], b["accs"][0], b["r"], b["accs"][1], 100, pos_all[lo:hi], neg_all[lo:hi], b["cfg"], b["ws"], b["loss"])
    for i, (x, y) in enumerate(zip(_host(a), _host(b))):
        assert_rows_close(x, y, "P = 0 epoch against triple_step, table %d" % i)
    assert abs(float(a["loss"].item()) - float(b["loss"].item())) <= 1e-5 * float(b["loss"].item())


DET_WORKER = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.environ["OEA_ROOT"]); sys.path.insert(0, os.path.join(os.environ["OEA_ROOT"], "tests"))
import torch
from openea_amd import ops
from test_iptranse_gpu import _path_only_problem, _run_epoch_and_loop, _setup, _train_step
assert ops.deterministic()
dev = ops.device()
runs = []
for _ in range(2):
    tables, b = _path_only_problem()
    s = _setup(tables, "SGD", dev)
    _train_step(s, b)
    torch.cuda.synchronize()
    runs.append(s["r"].cpu().numpy())
print("RESULT path_half same_bits=%d moved=%d" % (int(np.array_equal(runs[0], runs[1])),
                                                  int(not np.array_equal(runs[0][:, :100], tables[1].astype(np.float32)))))
tables, a, b = _run_epoch_and_loop(dev)
same = all(torch.equal(a[k], b[k]) for k in ("e", "r")) and all(torch.equal(x, y) for x, y in zip(a["accs"], b["accs"]))
print("RESULT epoch_vs_loop same_bits=%d" % int(same))
'''


def test_fixed_point_build_gives_the_same_bits():
    """libopenea_hip_det.so (OEA_STEP_DETERMINISTIC=1): A^T and the scratch in int64 fixed point -- two runs of the path half
    give identical bits of the relation table, and the epoch call equals the step loop bit for bit"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", DET_WORKER], env=dict(os.environ, OEA_ROOT=root, OEA_STEP_DETERMINISTIC="1"),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "RESULT path_half same_bits=1 moved=1" in p.stdout and "RESULT epoch_vs_loop same_bits=1" in p.stdout, p.stdout


@pytest.mark.parametrize("n1,n2,steps", [(966, 544, 18), (700, 0, 7)])
def test_path_sampler(n1, n2, steps):
    from openea_amd import ops
    dev = ops.device()
    rng = np.random.RandomState(2)
    rels = [np.arange(0, 267, dtype=np.int32), np.arange(267, 477, dtype=np.int32)]
    paths = [rng.randint(0, 267, (n1, 3)).astype(np.int32), rng.randint(267, 477, (n2, 3)).astype(np.int32)]
    # a weight that names its path: index + 1 on side 1, 100,000 + index on side 2 (exact in fp32)
    w = [np.arange(1, n1 + 1, dtype=np.float32), 100000 + np.arange(n2, dtype=np.float32)]
    args = [ops.to_ids(paths[0], dev), ops.to_vec(w[0], dev), ops.to_ids(paths[1], dev), ops.to_vec(w[1], dev),
            ops.to_ids(rels[0], dev), ops.to_ids(rels[1], dev)]
    P, num1 = ops.path_sample_dims(n1, n2, steps)
    assert P == (n1 + n2) // steps and num1 == int(n1 / (n1 + n2) * P)
    if (n1, n2, steps) == (966, 544, 18):
        assert (P, num1) == (83, 53)
    out = [t.cpu().numpy() for t in ops.path_sample_epoch(*args, steps, seed=9, epoch=3)]
    assert out[0].shape == (steps, P, 3) and out[1].shape == (steps, P) and out[2].shape == (steps, P)
    for s in range(steps):
        for side, (lo, hi) in enumerate(((0, num1), (num1, P))):
            ws = out[2][s, lo:hi]
            idx = (ws - 1 if side == 0 else ws - 100000).astype(np.int64)
            assert len(np.unique(idx)) == hi - lo                                       # no path twice in a step and side
            assert idx.min(initial=0) >= 0 and idx.max(initial=0) < max((n1, n2)[side], 1)
            assert np.array_equal(out[0][s, lo:hi], paths[side][idx])                   # every weight is its path's own
            assert np.isin(out[1][s, lo:hi], rels[side]).all()                          # r' from the path's own KG
    assert len(np.unique(out[1])) > 50                                                  # ... and spread over the list
    assert len({tuple(np.sort(out[2][s])) for s in range(steps)}) == steps              # steps draw different samples
    again = [t.cpu().numpy() for t in ops.path_sample_epoch(*args, steps, seed=9, epoch=3)]
    assert all(np.array_equal(x, y) for x, y in zip(out, again))
    other = [t.cpu().numpy() for t in ops.path_sample_epoch(*args, steps, seed=9, epoch=4)]
    assert not np.array_equal(out[2], other[2]) and not np.array_equal(out[1], other[1])


@pytest.mark.parametrize("call,bad", [("ptranse_step", b) for b in ("Adam", "Adadelta", "L1", "n_rel", "ld", "path_id", "neg_rel_id")]
                         + [("weighted_pair_step", b) for b in ("Adam", "Adadelta", "L1", "ld")])
def test_rejected_configurations_change_nothing(call, bad):
    """Adam / Adadelta / L1 / n_rel = 2049: OEA_EUNSUPPORTED, ld % 4 != 0: OEA_EINVAL, before anything is launched; a path id (or
    r') outside the table is found on the device: the path batch is left out and the wrapper raises from the flag.  (A step that
    also carries triples would still apply their half -- see include/openea_hip.h -- so the id cases run the path half alone.)"""
    from openea_amd import ops
    from openea_amd._lib import OpenEAHipError
    dev = ops.device()
    rng = np.random.RandomState(1)
    dim = 30
    n_rel = 2049 if bad == "n_rel" else 6
    tables = [rng.randn(50, dim) * 0.1, rng.randn(n_rel, dim) * 0.1]
    opt = bad if bad in ("Adam", "Adadelta") else "Adagrad"
    s = _setup(tables, opt, dev, loss_norm="L1" if bad == "L1" else "L2")
    if bad == "ld":                                             # ld = dim = 30, not a multiple of 4
        s["e"], s["r"] = s["e"][:, :dim].contiguous(), s["r"][:, :dim].contiguous()
        s["accs"] = [torch.full_like(s["e"], 0.1), torch.full_like(s["r"], 0.1)]
        s["ws"] = ops.step_workspace(50, n_rel, dim, dev)
        s["pws"] = ops.path_workspace(n_rel, dim, dev)
    ids = bad in ("path_id", "neg_rel_id")
    batch = dict(pos=np.zeros((0, 3), np.int32) if ids else np.array([[0, 1, 2], [3, 4, 5]]),
                 neg=np.zeros((0, 3), np.int32) if ids else np.array([[0, 1, 7], [9, 4, 5]]),
                 paths=np.array([[0, 1, 2], [3, 6 if bad == "path_id" else 3, 1]]),
                 neg_rel=np.array([4, -1 if bad == "neg_rel_id" else 5]), weight=np.array([1.0, 2.0]))
    e0, r0, a0 = s["e"].clone(), s["r"].clone(), [a.clone() for a in s["accs"]]
    with pytest.raises(OpenEAHipError) as err:
        if call == "ptranse_step":
            _train_step(s, batch)
        else:
            _align_step(s, dict(pos=batch["pos"], neg=batch["neg"], weight=np.array([0.75, 0.875])))
    msg = str(err.value)
    print(msg)
    assert "error %d" % (-1 if bad in ("ld", "path_id", "neg_rel_id") else -4) in msg and len(msg.split(":", 1)[1].strip()) > 10
    torch.cuda.synchronize()
    assert torch.equal(s["e"], e0) and torch.equal(s["r"], r0) and all(torch.equal(a, b) for a, b in zip(s["accs"], a0))
    assert float(s["loss"].item()) == 0.0
    if ids:                                                     # the flag was read and cleared
        assert int(s["pws"][1].item()) == 0


def test_end_to_end(tmp_path, capsys):
    import re
    from openea_amd.approaches import IPTransE
    from openea_amd.modules.base import initializers
    from openea_amd.modules.load.synth import make_kgs
    from openea_amd.run.default_args import get_args
    initializers.seed(20190719)
    kgs = make_kgs("small", mode="sharing", seed=0)
    d = 32
    model = IPTransE()
    model.set_args(get_args("IPTransE", output=str(tmp_path) + "/out/", training_data="synthetic/small/", dataset_division="fold1/",
                            dim=d, batch_size=2000, max_epoch=7, start_valid=2, eval_freq=2, bp_freq=2, sim_th=0.05))
    model.set_kgs(kgs)
    model.init()
    assert len(model.paths1) + len(model.paths2) > 0
    model.run()
    hits1 = model.valid("hits1")
    model.save()
    out = capsys.readouterr().out
    losses = {int(m.group(1)): float(m.group(2)) for m in re.finditer(r"epoch (\d+), avg\. triple loss: ([0-9.]+)", out)}
    assert sorted(losses) == [1, 2, 3, 4, 5, 6]                   # range(1, max_epoch)
    print("triple loss epoch 1 %.4f, epoch 6 %.4f; hits@1 %.2f" % (losses[1], losses[6], hits1))
    assert losses[6] < losses[1]
    assert re.search(r"epoch \d+, alignment loss: [0-9.]+", out), out[-2000:]
    assert "newly triples:" in out and "Training ends. Total time" in out
    assert np.isfinite(hits1)
    for t in (model.ent_embeds.var, model.rel_embeds.var, model._trainer.ent_acc, model._trainer.rel_acc,
              model._align_trainer.ent_acc, model._align_trainer.rel_acc):
        assert torch.isfinite(t).all()
    assert not torch.equal(model._align_trainer.ent_acc, torch.full_like(model._align_trainer.ent_acc, 0.1))
    ent = np.load(model.out_folder + "ent_embeds.npy")
    rel = np.load(model.out_folder + "rel_embeds.npy")
    assert ent.shape == (kgs.entities_num, d) and rel.shape == (kgs.relations_num, d) and ent.dtype == np.float32
    np.testing.assert_allclose(np.linalg.norm(ent, axis=1), 1.0, rtol=1e-5)
    assert model._trainer.t == 6 * model._epochs.triple_steps and model._align_trainer.t > 0
