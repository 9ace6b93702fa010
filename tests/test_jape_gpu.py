"""JAPE on the device: oea_sample_distinct, oea_log_uniform_sample_steps and the Attr2Vec step (csrc/attr2vec_step.hip),
oea_jape_step (csrc/jape_step.hip), the thresholded similarity CSR and oea_jape_sim_loss (csrc/sim_csr.hip) against the float64 restatements of test_jape_cpu.py, run to run in the fixed-point build,
and the configurations the entry points refuse."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_jape_cpu import (ATTR_CASES, ATTR_VARS, GOLDEN, attr_fixture_case, sim_fixture_csr, attr2vec_batch, attr2vec_loss_and_grads, attr2vec_reference_step, attr2vec_variables,  # noqa: E402
                           jape_batch, jape_reference_step, jape_sim_loss_reference, sample_distinct_reference, sim_csr_reference)
from test_proje_cpu import log_uniform_reference  # noqa: E402

E, R, N_POS = 300, 9, 64


# ---- 1. distinct draws ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,step", [(20190719, 0), (2 ** 40 + 5, 2 ** 33 + 7)])
@pytest.mark.parametrize("n", [1, 2, 1000, 2 ** 20 + 3])
def test_sample_distinct_equals_restatement(n, seed, step):
    from openea_amd import ops
    dev = ops.device()
    for m in sorted({1, n}):
        got = ops.sample_distinct(n, m, seed, step, dev=dev).cpu().numpy()
        assert got.dtype == np.int32 and got.shape == (m,)
        assert np.array_equal(got, sample_distinct_reference(n, m, seed, step)), (n, m)
        assert len(np.unique(got)) == m and got.min() >= 0 and got.max() < n


# ---- 1b. candidate sets for many steps ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_classes,n_sampled", [(14, 4), (37, 7), (700, 140), (8192, 64)])
def test_sample_steps_equal_the_single_step_sampler(n_classes, n_sampled):
    from openea_amd import ops
    dev = ops.device()
    assert ops.LOG_UNIFORM_STEPS_MAX_CLASSES == 8192
    seed, step0, steps = 20190719, 3, 5
    single = ops.LogUniformSampler(n_classes, n_sampled, seed, dev)
    ids, tries, logq, status = ops.log_uniform_sample_steps(n_classes, n_sampled, seed, step0, steps, single.thresholds)
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0
    for s in range(steps):
        i1, t1, q1 = single.sample(step0 + s)
        assert torch.equal(ids[s], i1) and int(tries[s]) == int(t1) and torch.equal(logq[s], q1), s      # bit for bit
    assert len({tuple(r) for r in ids.cpu().numpy().tolist()}) == steps


def test_sampler_failure_path_and_last_chunk():
    """n_classes = n_sampled = 8192 (the LDS limit): every class has to appear within 64 * 8192 tries = 128 chunks.  With this seed
    steps 1 and 2 get there (in the late chunks) and steps 3 and 4 miss one class: both ends of both kernels."""
    from openea_amd import ops
    from openea_amd._lib import OpenEAHipError
    from test_proje_cpu import classes_of, sampler_words, thresholds
    dev = ops.device()
    n, seed = ops.LOG_UNIFORM_STEPS_MAX_CLASSES, 20190719
    assert n == 8192
    assert len(np.unique(classes_of(sampler_words(seed, 3, 64 * n), thresholds(n)))) == n - 1      # the restatement itself misses one
    ref = {s: log_uniform_reference(n, n, seed, s) for s in (1, 2)}
    single = ops.LogUniformSampler(n, n, seed, dev)
    ids, tries, logq, status = ops.log_uniform_sample_steps(n, n, seed, 1, 4, single.thresholds)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, 0, 1, 1]
    for row, s in enumerate((1, 2)):
        ref_ids, ref_tries, ref_lq = ref[s]
        assert np.array_equal(ids[row].cpu().numpy(), ref_ids) and int(tries[row]) == ref_tries, s
        assert np.abs(logq[row].cpu().numpy().astype(np.float64) - ref_lq).max() <= 1e-6, s
    for row in (2, 3):
        assert torch.equal(ids[row], torch.arange(n, dtype=torch.int32, device=dev)), row
        assert int(logq[row].count_nonzero()) == 0 and int(tries[row]) == 1, row
    with pytest.raises(OpenEAHipError):
        single.sample(3)
    assert int(single.workspace.view(torch.int32)[:n].count_nonzero()) == 0       # a failed draw clears the table all the same
    i2, t2, q2 = single.sample(2)
    assert np.array_equal(i2.cpu().numpy(), ref[2][0]) and int(t2.item()) == ref[2][1]
    assert np.abs(q2.cpu().numpy().astype(np.float64) - ref[2][2]).max() <= 1e-6


def test_sample_steps_refuse_more_classes_than_fit():
    from openea_amd import ops
    from openea_amd._lib import OpenEAHipError
    dev = ops.device()
    n = ops.LOG_UNIFORM_STEPS_MAX_CLASSES + 1
    out = tuple(torch.zeros(s, dtype=t, device=dev) for s, t in (((2, 8), torch.int32), (2, torch.int64), ((2, 8), torch.float32),
                                                                   (2, torch.int32)))
    with pytest.raises(OpenEAHipError):
        ops.log_uniform_sample_steps(n, 8, 1, 0, 2, ops.log_uniform_thresholds(n, dev), out=out)
    torch.cuda.synchronize()
    assert all(int(t.count_nonzero()) == 0 for t in out)


# ---- 1c. the Attr2Vec step -----------------------------------------------------------------------------------------------------
A2V_A, A2V_S, A2V_B, A2V_SEED = 37, 7, 64, 20190719


def _a2v_absent(steps):
    """the largest attribute that none of the first `steps` candidate sets holds: kept out of the batches as well"""
    drawn = set()
    for s in range(steps):
        drawn |= set(int(c) for c in log_uniform_reference(A2V_A, A2V_S, A2V_SEED, s)[0])
    return max(a for a in range(A2V_A) if a not in drawn)


def _a2v_setup(variables, dev, max_s):
    from openea_amd import ops
    dim = variables[0].shape[1]
    v = [ops.to_table(variables[0], dev=dev), ops.to_table(variables[1], dev=dev), ops.to_vec(variables[2], dev)]
    return dict(v=v, accs=[torch.full_like(t, 0.1) for t in v], d=dim, ws=ops.attr2vec_workspace(v[0].shape[0], v[0].shape[1], max_s, dev),
                loss=torch.zeros(1, dtype=torch.float64, device=dev))


def _a2v_step(s, pairs, sampled, logq, tries, lr=0.05, phase=0):
    from openea_amd import ops
    ops.attr2vec_step(s["v"], s["accs"], s["d"], pairs, sampled, logq, tries, lr, s["ws"], s["loss"], phase=phase)


def _a2v_grads(s):
    from openea_amd import ops
    g = ops.attr2vec_grads(s["ws"])
    return [g[0][:, :s["d"]].cpu().numpy(), g[1][:, :s["d"]].cpu().numpy(), g[2].cpu().numpy()]


@pytest.mark.parametrize("dim", [75, 100, 128])
def test_attr2vec_gradients_equal_restatement(dim):
    """PHASE_GRAD against the float64 restatement: A = 37, S = 7, B = 64 (16 workgroups in the true half, 10 in the sampled one), one
    attribute in no pair and no candidate set.  Bound: 1e-4 of a gradient's largest entry -- an entry is a sum of at most B + S
    products of d-term fp32 dot products, so about (B + S + d) 2^-24 = 1.2e-5 relative in the worst order, with tenfold room.
    Nothing moves in this phase; the absent attribute's gradient rows are exactly zero."""
    from openea_amd import ops
    dev = ops.device()
    rng = np.random.RandomState(dim)
    variables = attr2vec_variables(rng, A2V_A, dim)
    sampler = ops.LogUniformSampler(A2V_A, A2V_S, A2V_SEED, dev)
    ids, tries, logq = sampler.sample(0)
    sampled, num_tries, _ = log_uniform_reference(A2V_A, A2V_S, A2V_SEED, 0)
    assert np.array_equal(ids.cpu().numpy(), sampled) and int(tries) == num_tries
    absent = _a2v_absent(1)
    pairs = attr2vec_batch(rng, A2V_A, A2V_B, sampled, absent)
    ref_loss, ref = attr2vec_loss_and_grads(variables, pairs, sampled, num_tries)
    s = _a2v_setup(variables, dev, A2V_S)
    before = [t.clone() for t in s["v"] + s["accs"]]
    for _ in range(2):                                   # a second gradient phase starts from a clean scratch
        s["loss"].zero_()
        _a2v_step(s, ops.to_ids(pairs, dev), ids, logq, tries, phase=ops.PHASE_GRAD)
    loss = float(s["loss"].item())
    print("Attr2Vec d=%d: loss %.9g (restatement %.9g, relative %.3g)" % (dim, loss, ref_loss, abs(loss - ref_loss) / ref_loss))
    assert abs(loss - ref_loss) <= 1e-5 * ref_loss
    for name, g, r in zip(ops.ATTR2VEC_VARS, _a2v_grads(s), ref):
        off = np.abs(g - r).max() / np.abs(r).max()
        print("Attr2Vec d=%d: %s gradient off by %.3g of its largest entry" % (dim, name, off))
        assert off <= 1e-4, name
        assert np.abs(g[absent]).max() == 0, name
    assert all(torch.equal(a, b) for a, b in zip(s["v"] + s["accs"], before))


def _a2v_run_steps(s, variables, steps, dev, rng, absent, ref=None, accs=None):
    from openea_amd import ops
    sampler = ops.LogUniformSampler(A2V_A, A2V_S, A2V_SEED, dev)
    loss_ref = 0.0
    for step in range(steps):
        ids, tries, logq = sampler.sample(step)
        sampled, num_tries, _ = log_uniform_reference(A2V_A, A2V_S, A2V_SEED, step)
        pairs = attr2vec_batch(rng, A2V_A, A2V_B, sampled, absent)
        if ref is not None:
            loss_ref += attr2vec_reference_step(ref, accs, pairs, sampled, num_tries, 0.05)
        _a2v_step(s, ops.to_ids(pairs, dev), ids, logq, tries)
    return loss_ref


@pytest.mark.parametrize("dim", [75, 128])
def test_attr2vec_adagrad_steps_equal_restatement(dim):
    """twenty Adagrad steps (lr 0.05) against the restatement, every row within the project's 1e-4; the attribute that is in no
    pair and no candidate set keeps the bits of its three rows and its accumulators stay at 0.1"""
    from _tol import assert_rows_close
    from openea_amd import ops
    dev = ops.device()
    rng = np.random.RandomState(100 + dim)
    variables = attr2vec_variables(rng, A2V_A, dim)
    absent = _a2v_absent(20)
    s = _a2v_setup(variables, dev, A2V_S)
    ref, accs = [v.copy() for v in variables], [np.full_like(v, 0.1) for v in variables]
    loss_ref = _a2v_run_steps(s, variables, 20, dev, rng, absent, ref, accs)
    loss = float(s["loss"].item())
    print("Attr2Vec d=%d: summed loss %.9g (restatement %.9g, relative %.3g)" % (dim, loss, loss_ref, abs(loss - loss_ref) / loss_ref))
    assert abs(loss - loss_ref) <= 1e-5 * loss_ref
    got = [s["v"][0][:, :dim].cpu().numpy(), s["v"][1][:, :dim].cpu().numpy(), s["v"][2].cpu().numpy()[:, None]]
    got_acc = [s["accs"][0][:, :dim].cpu().numpy(), s["accs"][1][:, :dim].cpu().numpy(), s["accs"][2].cpu().numpy()[:, None]]
    for name, g, a, r, ra, v0 in zip(ops.ATTR2VEC_VARS, got, got_acc, ref, accs, variables):
        r, ra, v0 = (x.reshape(len(x), -1) for x in (r, ra, v0))
        assert_rows_close(g, r, "Attr2Vec d=%d %s" % (dim, name))
        assert_rows_close(a, ra, "Attr2Vec d=%d %s accumulator" % (dim, name))
        assert np.array_equal(g[absent], v0[absent].astype(np.float32)) and (a[absent] == np.float32(0.1)).all(), name
        moved = np.linalg.norm(r - v0)
        off = np.linalg.norm(g - r)
        print("Attr2Vec d=%d %s: movement %.3g, off by %.3g" % (dim, name, moved, off))
        assert moved > 0 and off <= 1e-3 * moved + 20 * 2.0 ** -24 * np.linalg.norm(v0), name       # as the triple step's movement
    for t in s["v"][:2]:
        assert float(t[:, dim:].abs().sum()) == 0.0


def _a2v_epoch_vs_loop(dev, exact):
    """three steps of 48 pairs drawn from a list of 500: one oea_attr2vec_epoch call against the loop of single calls over
    sample_distinct / LogUniformSampler draws -> the two sets of tables"""
    from openea_amd import ops
    rng = np.random.RandomState(77)
    dim, steps, batch, step0 = 100, 3, 48, 11
    variables = attr2vec_variables(rng, A2V_A, dim)
    pairs = ops.to_ids(rng.randint(0, A2V_A, (500, 2)), dev)
    a = _a2v_setup(variables, dev, A2V_S)
    sampler = ops.LogUniformSampler(A2V_A, A2V_S, A2V_SEED, dev)
    for s in range(steps):
        idx = ops.sample_distinct(500, batch, A2V_SEED, step0 + s, dev=dev)
        ids, tries, logq = sampler.sample(step0 + s)
        _a2v_step(a, pairs[idx.long()].contiguous(), ids, logq, tries)
    b = _a2v_setup(variables, dev, A2V_S)
    bufs = ops.attr2vec_epoch(b["v"], b["accs"], dim, pairs, batch, steps, A2V_SEED, step0, sampler.thresholds, A2V_S, 0.05, b["ws"],
                              b["loss"])
    torch.cuda.synchronize()
    assert int(bufs[3].abs().sum()) == 0
    return a, b


def test_attr2vec_epoch_equals_the_step_loop():
    """the same draws, the same arithmetic: equal up to the order of the fp32 atomics (bit for bit in the fixed-point build, which
    test_fixed_point_build_gives_the_same_bits checks)"""
    from _tol import assert_rows_close
    from openea_amd import ops
    a, b = _a2v_epoch_vs_loop(ops.device(), False)
    la, lb = float(a["loss"].item()), float(b["loss"].item())
    assert la > 0 and abs(la - lb) <= 1e-6 * la
    for name, x, y in zip(ops.ATTR2VEC_VARS, a["v"] + a["accs"], b["v"] + b["accs"]):
        x, y = (t.cpu().numpy().reshape(A2V_A, -1) for t in (x, y))
        assert_rows_close(y, x, "epoch against step loop, " + name, tol=1e-6)
    assert not torch.equal(a["v"][0], ops.to_table(attr2vec_variables(np.random.RandomState(77), A2V_A, 100)[0], dev=ops.device()))


@pytest.mark.parametrize("bad", ["dim", "ld", "n_sampled", "batch", "max_sampled"])
def test_attr2vec_rejected_configurations_launch_nothing(bad):
    from openea_amd import ops
    from openea_amd._lib import OpenEAHipError
    dev = ops.device()
    rng = np.random.RandomState(2)
    dim = 129 if bad == "dim" else 30
    variables = attr2vec_variables(rng, A2V_A, dim)
    s = _a2v_setup(variables, dev, A2V_S)
    if bad == "ld":
        s["v"][:2] = [t[:, :dim].contiguous() for t in s["v"][:2]]
        s["accs"][:2] = [t[:, :dim].contiguous() for t in s["accs"][:2]]
        s["ws"]._shape = (A2V_A, dim, A2V_S)
    n_s = {"n_sampled": A2V_A + 1, "max_sampled": A2V_S + 1}.get(bad, A2V_S)
    if bad == "n_sampled":
        s["ws"] = ops.attr2vec_workspace(A2V_A, s["v"][0].shape[1], n_s, dev)
    ids = torch.arange(n_s, dtype=torch.int32, device=dev) % A2V_A
    logq = torch.zeros(n_s, dtype=torch.float32, device=dev)
    tries = torch.ones(1, dtype=torch.int64, device=dev)
    pairs = torch.zeros((0 if bad == "batch" else 4, 2), dtype=torch.int32, device=dev)
    before = [t.clone() for t in s["v"] + s["accs"]]
    with pytest.raises(OpenEAHipError):
        _a2v_step(s, pairs, ids, logq, tries)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(s["v"] + s["accs"], before))
    assert float(s["loss"].item()) == 0.0 and int(s["ws"].count_nonzero()) == 0


# ---- 2. the triple step --------------------------------------------------------------------------------------------------------
def _setup(tables, optimizer, dev, k, lr, l2n=True):
    from openea_amd import ops
    e, r = ops.to_table(tables[0], dev=dev), ops.to_table(tables[1], dev=dev)
    cfg = ops.make_step_cfg(loss="margin-based", optimizer=optimizer, lr=lr, neg_group_k=k, ent_l2_norm=l2n, rel_l2_norm=l2n)
    accs = [torch.full_like(t, 0.1) for t in (e, r)] if optimizer == "Adagrad" else [None, None]
    return dict(e=e, r=r, accs=accs, cfg=cfg, d=tables[0].shape[1], ws=ops.step_workspace(e.shape[0], r.shape[0], e.shape[1], dev),
                loss=torch.zeros(1, dtype=torch.float64, device=dev))


def _step(s, pos, neg, neg_alpha=0.1):
    from openea_amd import ops
    ops.jape_step(s["e"], s["accs"][0], s["r"], s["accs"][1], s["d"], pos, neg, neg_alpha, s["cfg"], s["ws"], s["loss"])


def _tables(rng, dim):
    return [rng.standard_normal((E, dim)) / np.sqrt(dim), rng.standard_normal((R, dim)) / np.sqrt(dim)]


@pytest.mark.parametrize("l2n", [True, False])
@pytest.mark.parametrize("optimizer", ["SGD", "Adagrad"])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("dim", [75, 100, 128])
def test_jape_steps_equal_restatement(dim, k, optimizer, l2n):
    """three steps of 64 positives (16 workgroups of four waves); dim = 75 has ld != dim, dim > 64 uses the second column of a
    lane pair's flush.  Rows are held with the project's tolerance; since that alone would pass a step that moved nothing, the
    movement is held as in test_rotate_distmult_gpu: |(got - start) - (ref - start)| <= 1e-3 |ref - start| + 1.5 * 2^-23 |start|
    (three roundings of an entry to fp32) in the Frobenius norm over the rows in use.  The last 20 entities and the last relation
    are in no triple: their rows keep their bits and their accumulators stay at 0.1."""
    from _tol import assert_rows_close
    from openea_amd import ops
    dev = ops.device()
    rng = np.random.RandomState(dim + 1000 * k + (7 if l2n else 0))
    tables = [t.astype(np.float32).astype(np.float64) for t in _tables(rng, dim)]
    lr = 0.01
    s = _setup(tables, optimizer, dev, k, lr, l2n)
    ref, accs = [t.copy() for t in tables], [np.full_like(t, 0.1) for t in tables]
    loss_ref = 0.0
    for _ in range(3):
        pos, neg = jape_batch(rng, E, R, N_POS, k)
        loss_ref += jape_reference_step(ref, accs, pos, neg, 0.1, lr, optimizer, ent_l2_norm=l2n, rel_l2_norm=l2n)
        _step(s, ops.to_ids(pos, dev), ops.to_ids(neg, dev))
    loss = float(s["loss"].item())
    what = "JAPE d=%d k=%d %s l2n=%s" % (dim, k, optimizer, l2n)
    print("%s: loss %.9g (restatement %.9g, relative %.3g)" % (what, loss, loss_ref, abs(loss - loss_ref) / abs(loss_ref)))
    assert abs(loss - loss_ref) <= 1e-5 * abs(loss_ref)
    got = [s["e"][:, :dim].cpu().numpy(), s["r"][:, :dim].cpu().numpy()]
    for i, (g, r) in enumerate(zip(got, ref)):
        assert_rows_close(g, r, "%s table %d" % (what, i))
    if optimizer == "Adagrad":
        got_acc = [a[:, :dim].cpu().numpy() for a in s["accs"]]
        for i, (g, r) in enumerate(zip(got_acc, accs)):
            assert_rows_close(g, r, "%s accumulator %d" % (what, i))
    for i, (g, r, t0) in enumerate(zip(got, ref, tables)):
        tail = 20 if i == 0 else 1
        assert np.array_equal(g[-tail:], t0[-tail:].astype(np.float32)), i
        if optimizer == "Adagrad":
            assert (got_acc[i][-tail:] == np.float32(0.1)).all(), i
        move_ref = r[:-tail] - t0[:-tail]
        off = np.linalg.norm((g[:-tail].astype(np.float64) - t0[:-tail]) - move_ref)
        bound = 1e-3 * np.linalg.norm(move_ref) + 1.5 * 2.0 ** -23 * np.linalg.norm(t0[:-tail])
        print("%s table %d: movement %.3g, off by %.3g (bound %.3g)" % (what, i, np.linalg.norm(move_ref), off, bound))
        assert np.linalg.norm(move_ref) > 0 and off <= bound, i
    for t in (s["e"], s["r"]):
        assert float(t[:, dim:].abs().sum()) == 0.0


DET_WORKER = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.environ["OEA_ROOT"]); sys.path.insert(0, os.path.join(os.environ["OEA_ROOT"], "tests"))
import torch
from openea_amd import ops
from test_jape_gpu import E, R, N_POS, _setup, _step, _tables, jape_batch
assert ops.deterministic()
dev = ops.device()
runs = []
for _ in range(2):
    rng = np.random.RandomState(7)
    tables = _tables(rng, 100)
    s = _setup(tables, "Adagrad", dev, 3, 0.01)
    for _ in range(3):
        pos, neg = jape_batch(rng, E, R, N_POS, 3)
        _step(s, ops.to_ids(pos, dev), ops.to_ids(neg, dev))
    torch.cuda.synchronize()
    runs.append((s["e"].cpu().numpy(), s["r"].cpu().numpy(), s["accs"][0].cpu().numpy(), s["accs"][1].cpu().numpy()))
moved = int(not np.array_equal(runs[0][0], ops.to_table(tables[0], dev=dev).cpu().numpy()))
print("RESULT JAPE same_bits=%d moved=%d" % (int(all(np.array_equal(a, b) for a, b in zip(*runs))), moved))
from test_jape_gpu import _a2v_epoch_vs_loop
runs = [_a2v_epoch_vs_loop(dev, True) for _ in range(2)]
flat = lambda s: [t.cpu().numpy() for t in s["v"] + s["accs"]]
same_runs = all(np.array_equal(x, y) for x, y in zip(flat(runs[0][1]), flat(runs[1][1])))
same_loop = all(np.array_equal(x, y) for x, y in zip(flat(runs[0][0]), flat(runs[0][1])))
print("RESULT Attr2Vec same_bits=%d epoch_equals_loop=%d" % (int(same_runs), int(same_loop)))
'''


def test_fixed_point_build_gives_the_same_bits():
    """libopenea_hip_det.so (OEA_STEP_DETERMINISTIC=1): two runs of three JAPE steps give bit-identical tables and accumulators;
    so do two runs of an Attr2Vec epoch, and there the epoch call leaves the bits of the loop of single steps"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", DET_WORKER], env=dict(os.environ, OEA_ROOT=root, OEA_STEP_DETERMINISTIC="1"),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "RESULT JAPE same_bits=1 moved=1" in p.stdout, p.stdout
    assert "RESULT Attr2Vec same_bits=1 epoch_equals_loop=1" in p.stdout, p.stdout


@pytest.mark.parametrize("bad", ["Adam", "n_neg", "dim", "ld", "neg_alpha"])
def test_jape_step_rejected_configurations_launch_nothing(bad):
    from openea_amd import ops
    from openea_amd._lib import OpenEAHipError
    dev = ops.device()
    rng = np.random.RandomState(1)
    dim = 129 if bad == "dim" else 30
    s = _setup([rng.randn(50, dim) * 0.1, rng.randn(6, dim) * 0.1], "Adagrad", dev, 1, 0.01)
    if bad == "ld":                                             # ld = dim = 30, not a multiple of 4
        s["e"] = s["e"][:, :dim].contiguous()
        s["r"] = s["r"][:, :dim].contiguous()
        s["accs"] = [torch.full_like(s["e"], 0.1), torch.full_like(s["r"], 0.1)]
        s["ws"] = ops.step_workspace(50, 6, dim, dev)
    if bad == "Adam":
        s["cfg"] = ops.make_step_cfg(loss="margin-based", optimizer="Adam", lr=0.01, neg_group_k=1)
        s["accs"] = [torch.zeros((2,) + tuple(t.shape), device=dev) for t in (s["e"], s["r"])]
    pos = ops.to_ids(np.array([[0, 1, 2], [3, 4, 5]]), dev)
    neg = ops.to_ids(np.array([[0, 1, 7], [9, 4, 5]] + ([[8, 4, 5]] if bad == "n_neg" else [])), dev)
    e0, r0 = s["e"].clone(), s["r"].clone()
    with pytest.raises(OpenEAHipError):
        _step(s, pos, neg, neg_alpha=-0.1 if bad == "neg_alpha" else 0.1)
    torch.cuda.synchronize()
    assert torch.equal(s["e"], e0) and torch.equal(s["r"], r0)
    assert float(s["loss"].item()) == 0.0 and int(s["ws"].count_nonzero()) == 0


# ---- 3. the thresholded CSR ----------------------------------------------------------------------------------------------------
def _csr_inputs():
    """67 x 131 products around the threshold 0.95; row 5 lies below it everywhere, row 50 above it everywhere"""
    rng = np.random.RandomState(11)
    d = 20
    e2 = np.abs(rng.standard_normal((131, d))) * 0.3 + 0.1
    e1 = np.abs(rng.standard_normal((67, d))) * 0.3 + 0.1
    prod = np.sort(e1 @ e2.T, axis=1)
    e1 *= (0.95 / (0.5 * (prod[:, 65] + prod[:, 66])))[:, None]    # every other row straddles the threshold, between two products
    e1[5] = -0.2
    e1[50] = 1.5
    return e1.astype(np.float32).astype(np.float64), e2.astype(np.float32).astype(np.float64), d


def test_sim_csr_equals_numpy():
    """two row blocks (40 + 27 rows).  The kept set is only defined where no product sits on the threshold: the inputs keep every
    float64 product 1e-5 away from it (asserted), forty times the rounding of a 20-term fp32 dot product of this size
    (20 * 2^-24 * sum |a b| < 2.4e-7 * sum |a b|, asserted below 1e-5 / 4 for the rows that straddle)."""
    from openea_amd import ops
    dev = ops.device()
    e1, e2, d = _csr_inputs()
    thr = 0.95
    indptr, col, val, dense = sim_csr_reference(e1, e2, thr)
    assert np.abs(dense - np.float32(thr)).min() > 1e-5
    err = d * 2.0 ** -24 * (np.abs(e1) @ np.abs(e2).T)
    straddle = np.setdiff1d(np.arange(67), [5, 50])
    assert err[straddle].max() < 2.5e-6
    counts = np.diff(indptr)
    assert counts[5] == 0 and counts[50] == 131 and 0 < counts[straddle].min() and counts[straddle].max() < 131
    g_indptr, g_col, g_val = ops.sim_csr(ops.to_table(e1, dev=dev), ops.to_table(e2, dev=dev), d, thr, block_rows=40)
    assert g_indptr.dtype == torch.int64 and g_col.dtype == torch.int32 and g_val.dtype == torch.float32
    assert np.array_equal(g_indptr.cpu().numpy(), indptr)
    assert np.array_equal(g_col.cpu().numpy(), col)
    off = np.abs(g_val.cpu().numpy().astype(np.float64) - val)
    bound = err[dense >= thr]
    print("sim_csr: nnz %d, values off by at most %.3g (bound %.3g)" % (len(col), off.max(), bound.max()))
    assert (off <= bound + 2.0 ** -24 * np.abs(val)).all()          # the dot product's rounding + the result's own
    # one block of all rows gives the same arrays
    one = ops.sim_csr(ops.to_table(e1, dev=dev), ops.to_table(e2, dev=dev), d, thr, block_rows=4096)
    assert all(torch.equal(a, b) for a, b in zip(one, (g_indptr, g_col, g_val)))


# ---- 4. the similarity loss ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [75, 128])
def test_sim_loss_equals_restatement(dim):
    """12 rows of ref1 against 320 of ref2: row 3 is empty (its term is |l2n row|^2 = 1), row 8 holds 300 entries, a sampled
    position repeats; nothing but the loss is written"""
    from openea_amd import ops
    dev = ops.device()
    rng = np.random.RandomState(dim)
    n_ent, n1, n2 = 500, 12, 320
    ent = (rng.standard_normal((n_ent, dim)) * 0.3).astype(np.float32).astype(np.float64)
    ref1, ref2 = rng.permutation(n_ent)[:n1].astype(np.int32), rng.permutation(n_ent)[:n2].astype(np.int32)
    counts = rng.randint(1, 9, n1)
    counts[3], counts[8] = 0, 300
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(n2, c, replace=False)) for c in counts]).astype(np.int32)
    val = (0.95 + 0.05 * rng.rand(len(col))).astype(np.float32)
    rows = np.array([0, 3, 8, 8, 11, 5, 1, 2, 4], np.int32)
    beta = 0.001
    want = jape_sim_loss_reference(ent, ref1, ref2, indptr, col, val.astype(np.float64), rows, float(np.float32(beta)))
    table = ops.to_table(ent, dev=dev)
    before = table.clone()
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    args = (table, dim, ops.to_ids(ref1, dev), ops.to_ids(ref2, dev), torch.from_numpy(indptr).to(dev), ops.to_ids(col, dev),
            ops.to_vec(val, dev))
    ops.jape_sim_loss(*args, ops.to_ids(rows, dev), beta, loss)
    got = float(loss.item())
    print("sim loss d=%d: %.12g (restatement %.12g, relative %.3g)" % (dim, got, want, abs(got - want) / want))
    assert abs(got - want) <= 1e-6 * want
    assert torch.equal(table, before)
    ops.jape_sim_loss(*args, ops.to_ids(np.array([3], np.int32), dev), 1.0, loss)       # the empty row alone adds 1
    assert abs(float(loss.item()) - got - 1.0) <= 1e-6


def test_sim_entry_points_reject_before_any_launch():
    from openea_amd import ops
    from openea_amd._lib import OpenEAHipError
    dev = ops.device()
    with pytest.raises(OpenEAHipError):
        ops.sample_distinct(5, 6, 1, 0, dev=dev)
    with pytest.raises(OpenEAHipError):
        ops.sample_distinct(2 ** 31, 1, 1, 0, dev=dev)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    ids = ops.to_ids(np.array([0, 1], np.int32), dev)
    indptr = torch.zeros(3, dtype=torch.int64, device=dev)
    empty_i, empty_f = torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.float32, device=dev)
    for shape, dim in (((4, 132), 129), ((4, 30), 30)):                       # dim > 128; ld % 4 != 0
        with pytest.raises(OpenEAHipError):
            ops.jape_sim_loss(torch.ones(shape, device=dev), dim, ids, ids, indptr, empty_i, empty_f, ids, 1.0, loss)
    with pytest.raises(OpenEAHipError):
        ops.sim_csr(torch.ones((4, 30), device=dev), torch.ones((4, 30), device=dev), 30, 0.5)
    torch.cuda.synchronize()
    assert float(loss.item()) == 0.0


# ---- 5. the reference's own graphs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ATTR_CASES)
def test_attr2vec_gradients_equal_reference_graph(case):
    """PHASE_GRAD on the fixture's batch (a repeated input, a repeated label, a label among the samples, input == label): 2e-5 on the
    loss and 1e-3 of a gradient's largest entry, as the other fp32 steps are held to their finite-difference fixtures"""
    from openea_amd import ops
    dev = ops.device()
    z = np.load(GOLDEN)
    variables, pairs, sampled, num_tries = attr_fixture_case(z, case)
    n_attr, d, n_b, n_s = (int(x) for x in z[case + "_shape"])
    sampler = ops.LogUniformSampler(n_attr, n_s, 20190719, dev)
    ids, tries, logq = sampler.sample(0)
    assert np.array_equal(ids.cpu().numpy(), sampled) and int(tries) == num_tries
    s = _a2v_setup(variables, dev, n_s)
    _a2v_step(s, ops.to_ids(pairs, dev), ids, logq, tries, phase=ops.PHASE_GRAD)
    loss, ref_loss = float(s["loss"].item()), float(z[case + "_loss"][0])
    print("%s: loss %.9g (fixture %.9g, relative %.3g)" % (case, loss, ref_loss, abs(loss - ref_loss) / ref_loss))
    assert abs(loss - ref_loss) <= 2e-5 * ref_loss
    for name, g in zip(ATTR_VARS, _a2v_grads(s)):
        ref = z["%s_grad_%s" % (case, name)]
        off = np.abs(g - ref).max() / np.abs(ref).max()
        print("%s: %s gradient off by %.3g of its largest entry" % (case, name, off))
        assert off <= 1e-3, name


def test_jape_step_equals_reference_graph():
    """one SGD step on the fixture's batch (k = 2, a negative that shares rows with its positive, h == t): the update IS lr * gradient"""
    from openea_amd import ops
    dev = ops.device()
    z = np.load(GOLDEN)
    tables = [z["triple_d5_var_ent_embeds"], z["triple_d5_var_rel_embeds"]]
    lr = 0.01
    s = _setup(tables, "SGD", dev, 2, lr)
    _step(s, ops.to_ids(z["triple_d5_pos"], dev), ops.to_ids(z["triple_d5_neg"], dev), neg_alpha=float(z["triple_d5_neg_alpha"][0]))
    loss, ref_loss = float(s["loss"].item()), float(z["triple_d5_loss"][0])
    print("triple_d5: loss %.9g (fixture %.9g, relative %.3g)" % (loss, ref_loss, abs(loss - ref_loss) / ref_loss))
    assert abs(loss - ref_loss) <= 2e-5 * ref_loss
    for name, t0, got in zip(("ent_embeds", "rel_embeds"), tables, (s["e"], s["r"])):
        g = (t0 - got[:, :5].cpu().numpy().astype(np.float64)) / lr
        ref = z["triple_d5_grad_" + name]
        off = np.abs(g - ref).max() / np.abs(ref).max()
        print("triple_d5: %s gradient off by %.3g of its largest entry" % (name, off))
        assert off <= 1e-3, name


def test_sim_loss_equals_reference_graph():
    from openea_amd import ops
    dev = ops.device()
    z = np.load(GOLDEN)
    indptr, col, val = sim_fixture_csr(z)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    args = (ops.to_table(z["triple_d5_var_ent_embeds"], dev=dev), 5, ops.to_ids(z["sim_d5_ref1"], dev), ops.to_ids(z["sim_d5_ref2"], dev),
            torch.from_numpy(indptr).to(dev), ops.to_ids(col, dev), ops.to_vec(val, dev))
    ops.jape_sim_loss(*args, ops.to_ids(z["sim_d5_idx"], dev), float(z["sim_d5_beta"][0]), loss)
    got, want = float(loss.item()), float(z["sim_d5_loss"][0])
    print("sim_d5: %.12g (fixture %.12g)" % (got, want))
    assert abs(got - want) <= 1e-6 * want


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------------
def test_end_to_end(tmp_path, capsys):
    """make_kgs("small", attributes=True): 3 attribute epochs, 5 joint epochs.  The three losses are finite, launch_sim_1epo leaves
    the entity table's bits alone (the reference never runs sim_optimizer), the triple loss falls, test() reports metrics."""
    import re
    from openea_amd.approaches import JAPE
    from openea_amd.modules.base import initializers
    from openea_amd.modules.load.synth import make_kgs
    from openea_amd.run.default_args import get_args
    initializers.seed(20190719)
    kgs = make_kgs("small", mode="sharing", seed=0, attributes=True)
    model = JAPE()
    model.set_args(get_args("JAPE", output=str(tmp_path) + "/out/", training_data="synthetic/small/", dataset_division="fold1/", dim=32,
                            batch_size=2000, attr_max_epoch=3, max_epoch=5, start_valid=5, eval_freq=5, sub_mat_size=500))
    model.set_kgs(kgs)
    model.init()
    e0 = model.ent_embeds.var.clone()
    model.run_attr2vec()
    n_ref = len(model.ref_entities1)
    assert model.attr_sim_mat[0].shape == (n_ref + 1,)
    # three epochs do not bring two KGs' attribute rows to 0.95 of each other: for the rest of the test keep the top 1 % of the
    # matrix, whatever its values are
    dense = model.attr2vec.eval_sim_mat()
    thr = float(np.quantile(dense, 0.99))
    model.attr_sim_mat = model.attr2vec.eval_sim_csr(thr, block_rows=1000)
    indptr, col, val = model.attr_sim_mat
    assert dense.shape == (n_ref, len(model.ref_entities2)) and int((dense >= np.float32(thr)).sum()) == col.numel() == int(indptr[-1]) > 0
    assert float(val.min()) >= np.float32(thr)
    assert torch.equal(model.ent_embeds.var, e0)
    sim0 = model.launch_sim_1epo(0)
    assert np.isfinite(sim0) and sim0 > 0 and torch.equal(model.ent_embeds.var, e0)              # bits before and after
    model.run_attr2vec = lambda: None                                                            # the attribute half has run
    model.run()
    model.test()
    out = capsys.readouterr().out
    attr = [float(x) for x in re.findall(r"epoch \d+, attribute loss: ([-\d.naninf]+),", out)]
    triple = [float(x) for x in re.findall(r"epoch \d+, avg. triple loss: ([-\d.naninf]+),", out)]
    sim = [float(x) for x in re.findall(r"epoch \d+, sim loss: ([-\d.naninf]+),", out)]
    print(attr, triple, sim)
    assert len(attr) == 3 and len(triple) == 5 and len(sim) == 6
    assert all(np.isfinite(v) for v in attr + triple + sim) and attr[-1] < attr[0] and triple[-1] < triple[0]
    assert "Training attributes ends. Total time" in out and "Joint training:" in out and "Training ends. Total time" in out
    assert "accurate results: hits@[1, 5, 10, 50]" in out
    assert torch.isfinite(model.ent_embeds.var).all() and not torch.equal(model.ent_embeds.var, e0)


# ---- 7. entity rows from attributes, the epoch call's edges -------------------------------------------------------------------
@pytest.mark.parametrize("which", ["host_selected", "host_selected_few"])
def test_ent_embeds_from_attributes_equal_the_reference(which):
    """get_ent_embeds_from_attributes (oea_spmm_csr with 1 / count, then the sklearn normalisation) against what the reference's
    function returned for the same KG pair, attribute table and selection.  Bound per entry: the mean of at most A = 54 fp32 rows
    and one normalisation, (54 + 6 + 2) 2^-24 = 3.7e-6 of a unit row, taken as 4e-6.  With three selected attributes most entities
    have none: those rows are zero in every bit."""
    from openea_amd.approaches import attr2vec as a2v
    from openea_amd.modules.load.synth import make_kgs
    z = np.load(GOLDEN)
    kgs = make_kgs("tiny", mode="sharing", seed=0, attributes=True)
    want = z["host_ent_mat" + which[len("host_selected"):]]
    got = a2v.get_ent_embeds_from_attributes(kgs, z["host_attr_embeds"], set(z[which].tolist()))
    assert got.shape == want.shape == (kgs.entities_num, 6) and got.dtype == np.float32
    zero = np.abs(want).sum(1) == 0
    assert zero.any() == (which == "host_selected_few") and not zero.all()
    assert np.array_equal(got[zero], np.zeros_like(got[zero]))
    off = np.abs(got.astype(np.float64) - want).max()
    print("%s: %d zero rows, entries off by at most %.3g" % (which, int(zero.sum()), off))
    assert off <= 4e-6
    np.testing.assert_allclose(np.linalg.norm(got[~zero], axis=1), 1.0, rtol=0, atol=1e-6)


def test_epoch_refusals_and_no_steps():
    """more attributes than the candidate sampler's table holds: refused without a launch; no steps: nothing happens, whatever the
    list holds (fewer pairs than one batch: the reference runs no step either); the apply phase needs neither batch nor candidates"""
    from openea_amd import ops
    from openea_amd._lib import OpenEAHipError
    dev = ops.device()
    n = ops.LOG_UNIFORM_STEPS_MAX_CLASSES + 1
    v = [torch.ones((n, 4), device=dev), torch.ones((n, 4), device=dev), torch.zeros(n, device=dev)]
    accs = [torch.full_like(t, 0.1) for t in v]
    ws = ops.attr2vec_workspace(n, 4, 2, dev)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    pairs = torch.zeros((8, 2), dtype=torch.int32, device=dev)
    before = [t.clone() for t in v + accs]
    with pytest.raises(OpenEAHipError):
        ops.attr2vec_epoch(v, accs, 4, pairs, 4, 2, 1, 0, ops.log_uniform_thresholds(n, dev), 2, 0.01, ws, loss)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(v + accs, before)) and int(ws.count_nonzero()) == 0 and float(loss.item()) == 0.0
    s = _a2v_setup(attr2vec_variables(np.random.RandomState(0), A2V_A, 16), dev, A2V_S)
    before = [t.clone() for t in s["v"] + s["accs"]]
    thr = ops.log_uniform_thresholds(A2V_A, dev)
    ops.attr2vec_epoch(s["v"], s["accs"], 16, pairs[:3].contiguous(), 64, 0, 1, 0, thr, A2V_S, 0.01, s["ws"], s["loss"])
    empty = torch.zeros((0, 2), dtype=torch.int32, device=dev)
    _a2v_step(s, empty, empty[:, 0].contiguous(), torch.zeros(0, device=dev), torch.ones(1, dtype=torch.int64, device=dev),
              phase=ops.PHASE_APPLY)                     # nothing was flagged: a no-op that is accepted
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(s["v"] + s["accs"], before)) and float(s["loss"].item()) == 0.0


def test_a_step_whose_draw_failed_changes_nothing():
    """n_classes = n_sampled = 8192 asks for EVERY class; at seed 2 the 64 x 8192 draws of step 0 show 8,191 of them (the numpy
    restatement's count), those of step 1 all.  The epoch call over both steps reports status (1, 0) and leaves what the single
    step 1 leaves: the failed step's kernels returned on its status word."""
    from _tol import assert_rows_close
    from openea_amd import ops
    dev = ops.device()
    n, dim, batch, seed = 8192, 8, 32, 2
    rng = np.random.RandomState(4)
    variables = attr2vec_variables(rng, n, dim)
    pairs = ops.to_ids(rng.randint(0, n, (100, 2)), dev)
    a = _a2v_setup(variables, dev, n)
    sampler = ops.LogUniformSampler(n, n, seed, dev)
    ids, tries, logq = sampler.sample(1)
    idx = ops.sample_distinct(100, batch, seed, 1, dev=dev)
    _a2v_step(a, pairs[idx.long()].contiguous(), ids, logq, tries)
    b = _a2v_setup(variables, dev, n)
    b["ws"] = a["ws"]                                   # one 0.8 GB workspace for both runs: a step leaves it clean
    bufs = ops.attr2vec_epoch(b["v"], b["accs"], dim, pairs, batch, 2, seed, 0, sampler.thresholds, n, 0.05, b["ws"], b["loss"])
    torch.cuda.synchronize()
    assert bufs[3].tolist() == [1, 0]
    assert abs(float(a["loss"].item()) - float(b["loss"].item())) <= 1e-6 * float(a["loss"].item())
    for name, x, y in zip(ops.ATTR2VEC_VARS, a["v"] + a["accs"], b["v"] + b["accs"]):
        assert_rows_close(y.cpu().numpy().reshape(n, -1), x.cpu().numpy().reshape(n, -1), "failed step skipped, " + name, tol=1e-6)
    assert not torch.equal(b["v"][0], ops.to_table(variables[0], dev=dev))
