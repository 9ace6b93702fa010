"""The relation order of the epoch plan, and the planned step that sums a workgroup's relation rows before the atomics.

`oea_step_plan_build` leaves `rel_order`: every step's positives (index inside the batch) in stable ascending order of relation id.
`triple_wave<..., PLAN = true>` maps wave slot q to positive `rel_order[q]`, so the 8 waves of a workgroup nearly always hold one
relation; they leave their relation rows in LDS and the first wave of every (workgroup, relation) group issues ONE row of atomics.
`OEA_STEP_REL_ORDER=0` is batch order and one row of atomics per positive.

  * `rel_order` == `np.argsort(relations of the batch, kind="stable")`, step by step, and the plan's other arrays do not depend on
    the switch;
  * the planned step against the C oracle (`oracle.cport.triple_step`), teacher-forced, with the helpers and the bounds of
    tests/test_step_plan_gpu.py (rows of both tables at the project's 1e-4, accumulators, loss): the default dispatch at the 100K
    shape over the last step of one epoch and the first of the next (a new plan in the same buffer), and every fragment count at a
    small shape under OEA_STEP_PLAN=2;
  * at the 100K shape the order leaves fewer than 25 % as many (workgroup of 8, relation) groups as positives, batch order more
    than 75 %: what the kernel sums is what the issue counted;
  * switch off == default within the 2e-6 of `test_planned_epochs_equal_the_atomic_epochs`.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_step_plan_gpu as sp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    from openea_amd import ops as _ops
    _ops.lib()   # raises loudly if the HIP library / GPU is missing
    return _ops


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs: test_step_plan_gpu.make_batches, with the relations of a case's first batch rewritten where the case asks for it
# ---------------------------------------------------------------------------------------------------------------------------------

_make_batches = sp.make_batches


def make_batches(c):
    """c["rel_mode"] == "single": every positive of the first batch (and its negatives) carries relation 0 -- a single-relation batch:
    every workgroup is one group.  The planted entry that is no corruption of its positive keeps its own relation."""
    pos, neg, offsets = _make_batches(c)
    if c.get("rel_mode") == "single":
        k, hi = c["k"], int(offsets[1])
        foreign = (neg[:hi * k] != np.repeat(pos[:hi], k, 0))[:, 1]
        pos[:hi, 1] = 0
        neg[:hi * k][~foreign, 1] = 0
        assert len(np.unique(pos[:hi, 1])) == 1
    return pos, neg, offsets


@pytest.fixture(autouse=True)
def _own_batches(monkeypatch):
    """the helpers of test_step_plan_gpu draw their batches through its module-level name; cases without "rel_mode" get what it gives"""
    monkeypatch.setattr(sp, "make_batches", make_batches)
    monkeypatch.setattr(sp, "WORKER", WORKER)


WORKER = r'''
import os, sys
sys.path[:0] = [os.environ["OEA_ROOT"], os.path.join(os.environ["OEA_ROOT"], "tests")]
import test_rel_order_gpu as t
t.sp.make_batches = t.make_batches
t.worker_entry()
'''


def worker_entry():
    if os.environ.get("OEA_REL_MODE") == "arrays":
        arrays_worker()
    elif os.environ.get("OEA_REL_MODE") == "free":
        free_worker()
    else:
        sp.worker_main()


def run_script(env_extra, timeout=900):
    env = dict(os.environ, OEA_ROOT=ROOT)
    for key in ("OEA_STEP_DETERMINISTIC", "OEA_STEP_WAVE", "OEA_STEP_PLAN", "OEA_APPLY_G16", "OEA_APPLY_V4", "OEA_STEP_RUNTIME_KIND",
                "OEA_STEP_WAVE_BLOCK", "OEA_STEP_REL_ORDER"):
        env.pop(key, None)
    env.update(env_extra)
    p = subprocess.run([sys.executable, "-c", WORKER], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    assert p.returncode == 0, p.stdout.decode(errors="replace")[-3000:]


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. rel_order against numpy
# ---------------------------------------------------------------------------------------------------------------------------------

SIZES = [1000, 0, 333, 8, 2501, 1, 77]            # ragged, one empty, multiples of 8 and not
N_RELS = (1, 17, 700, 5000, 3000000)              # (the plan is built from the ids alone: no relation table this size exists)


def order_inputs(n_rel):
    rng = np.random.RandomState(900 + n_rel)
    n_ent, k = 3000, 5
    offsets = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    n = int(offsets[-1])
    if n_rel <= 1000:
        w = 1.0 / np.arange(1, n_rel + 1)                            # Zipf weights, as in the synthetic KGs
        rel = rng.choice(n_rel, n, p=w / w.sum())
    else:
        rel = rng.randint(0, n_rel, n)                               # (the build sorts by 10-bit digits: two and three of them)
        rel[::7] = rel[3]                                            # ... with ties
    pos = np.stack([rng.randint(0, n_ent, n), rel, rng.randint(0, n_ent, n)], 1).astype(np.int32)
    neg = np.repeat(pos, k, 0)
    side = np.repeat(rng.rand(n) < 0.5, k)
    neg[side, 0] = rng.randint(0, n_ent, int(side.sum()))
    neg[~side, 2] = rng.randint(0, n_ent, int((~side).sum()))
    return pos, neg, offsets, k, n_ent


def build_plan(ops, n_rel):
    import torch
    pos, neg, offsets, k, n_ent = order_inputs(n_rel)
    dims = (len(pos), len(SIZES), max(SIZES), n_ent, 36)
    plan = ops.step_plan_buffer(*dims, dev=ops.device())
    plan.fill_(0xA5)                                                  # what an earlier epoch left there
    ops.step_plan_build(ops.to_ids(pos), ops.to_ids(neg), k, torch.from_numpy(offsets).to(ops.device()), *dims, plan)
    torch.cuda.synchronize()
    out = ops.step_plan_arrays(plan, *dims)
    out["rel_order"] = ops.step_plan_rel_order(plan, *dims)
    return pos, offsets, out


def arrays_worker():
    from openea_amd import ops
    ops.lib()
    out = {}
    for n_rel in N_RELS:
        for key, v in build_plan(ops, n_rel)[2].items():
            out["%d_%s" % (n_rel, key)] = np.asarray(v)
    np.savez(os.environ["OEA_OUT"], **out)


def stable_order(pos, offsets):
    return np.concatenate([np.argsort(pos[int(a):int(b), 1], kind="stable") for a, b in zip(offsets[:-1], offsets[1:])]).astype(np.uint32)


def test_rel_order_is_the_stable_argsort_of_every_batch(ops, tmp_path):
    """n_rel 1 (the order is the identity), 17, 700, 5,000 and 3,000,000; batches of 1000, 0, 333, 8, 2501, 1 and 77 positives.  The arrays the plan had
    before (`ops.step_plan_arrays`) and rel_order itself are the same bits in a process under OEA_STEP_REL_ORDER=0: the switch
    changes what the scoring kernel does with the order, not the plan."""
    out = str(tmp_path / "arrays_off.npz")
    run_script(dict(OEA_REL_MODE="arrays", OEA_OUT=out, OEA_STEP_REL_ORDER="0"))
    off = np.load(out)
    for n_rel in N_RELS:
        pos, offsets, got = build_plan(ops, n_rel)
        ref = stable_order(pos, offsets)
        for s in range(len(SIZES)):
            a, b = int(offsets[s]), int(offsets[s + 1])
            assert np.array_equal(got["rel_order"][a:b], ref[a:b]), "n_rel %d, step %d" % (n_rel, s)
        if n_rel == 1:
            assert np.array_equal(ref[:SIZES[0]], np.arange(SIZES[0]))
        for key, v in got.items():
            assert np.array_equal(np.asarray(v), off["%d_%s" % (n_rel, key)]), "n_rel %d: '%s' depends on OEA_STEP_REL_ORDER" % (n_rel, key)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the default dispatch at the 100K shape, across an epoch boundary; the groups the kernel sums
# ---------------------------------------------------------------------------------------------------------------------------------


def groups_per_step(rel, order, wg=8):
    """(workgroup of `wg` consecutive wave slots, relation) groups of one step: the rows of relation atomics the step issues when
    every positive has an active triple"""
    r = rel[order]
    pad = (-len(r)) % wg
    blocks = np.concatenate([r, np.full(pad, -1, r.dtype)]).reshape(-1, wg)
    return sum(len(np.unique(b[b >= 0])) for b in blocks)


def zipf_relations(c, pos, neg):
    """the relations of a case's positives (and of their negatives) redrawn from the Zipf law of the synthetic KGs (weight 1 / rank)"""
    rng = np.random.RandomState(50 + c["seed"])
    w = 1.0 / np.arange(1, c["n_rel"] + 1)
    foreign = (neg != np.repeat(pos, c["k"], 0))[:, 1]
    pos[:, 1] = rng.choice(c["n_rel"], len(pos), p=w / w.sum())
    neg[~foreign, 1] = np.repeat(pos[:, 1], c["k"])[~foreign]


def test_default_dispatch_at_the_100k_shape_across_an_epoch_boundary(ops, monkeypatch, capsys):
    """EN-FR-100K shape (200,000 entities, 700 relations with Zipf weights, d 100, k 10), no switch set: `triple_wave<2, 0, 10, true>`
    with the order, `apply_step_plan<16, 7, true>`.  Epoch A = batches of 20,000 and 19,825; epoch B = 19,825 and 20,000 other positives:
    its plan is built into the SAME buffer, over A's.  Four teacher-forced Adagrad steps; the tables, the accumulators, the workspace
    and the plan buffer carry over the boundary.  From the device's rel_order: the (workgroup of 8, relation) groups of every step
    are below 25 % of its positives (the issue counted 15.6 % on the bench's KG), in batch order above 75 % (84 %)."""
    def zipf_batches(c):
        pos, neg, offsets = _make_batches(c)
        zipf_relations(c, pos, neg)
        return pos, neg, offsets
    monkeypatch.setattr(sp, "make_batches", zipf_batches)
    ca = sp.case("100k-A", n_ent=200000, n_rel=700, d=100, sizes=(20000, 19825), k=10, neg_margin=3.0, seed=7)
    cb = sp.case("100k-B", n_ent=200000, n_rel=700, d=100, sizes=(19825, 20000), k=10, neg_margin=3.0, seed=8)
    tables = sp.make_tables(ca)
    expect = ("outside", "listed", "hubs", "merge", "scan")
    with capsys.disabled():
        print()
        run = sp.DeviceRun(ops, ca, *zipf_batches(ca), tables)
        assert run.supported, "the default dispatch does not choose the plan at the 100K shape"

        def run_call(j, lo, hi, forced):
            if forced is not None:
                run.set_state(forced)
            return run.run(lo, hi)
        _, traj = sp.check_case("100K shape, epoch A", ca, run_call, expect, tables)
        for c, r in ((ca, run),):
            check_groups(ops, c, r, zipf_batches(c))
        # epoch B: other batches, the same tensors, the plan rebuilt into the same buffer
        nxt = sp.DeviceRun(ops, cb, *zipf_batches(cb), tables)
        assert nxt.plan.numel() == run.plan.numel()
        for name in ("e", "ea", "r", "ra", "ws", "plan"):
            setattr(nxt, name, getattr(run, name))
        run = nxt
        tables_b = traj[-1][2]                                       # the oracle's state after epoch A
        run.set_state(tables_b)
        sp.check_case("100K shape, epoch B", cb, run_call, expect, tables_b)
        check_groups(ops, cb, run, zipf_batches(cb))


def check_groups(ops, c, run, batches):
    pos, _, offsets = batches
    dims = (len(pos), len(c["sizes"]), int(np.diff(offsets).max()), c["n_ent"], run.ld)
    order = ops.step_plan_rel_order(run.plan, *dims)
    assert np.array_equal(order, stable_order(pos, offsets))
    for s in range(len(c["sizes"])):
        a, b = int(offsets[s]), int(offsets[s + 1])
        rel = pos[a:b, 1]
        sorted_groups, batch_groups = groups_per_step(rel, order[a:b].astype(np.int64)), groups_per_step(rel, np.arange(b - a))
        print("%s step %d: %d positives, %d (workgroup, relation) groups in relation order (%.1f %%), %d in batch order (%.1f %%)"
              % (c["name"], s, b - a, sorted_groups, 100.0 * sorted_groups / (b - a), batch_groups, 100.0 * batch_groups / (b - a)))
        assert sorted_groups < 0.25 * (b - a)
        assert batch_groups > 0.75 * (b - a)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. every fragment count at a small shape under OEA_STEP_PLAN=2
# ---------------------------------------------------------------------------------------------------------------------------------


def small_cases():
    """ld 36, 76 (d 75), 100 and 200 = 1, 2, 2 and 4 fragments of 64 lanes (at ld 200 a workgroup is 4 waves); k 10 (the KT = 10
    instance) and 5; L2 and L1 (an L1 score of unit rows is about 1.4 sqrt(d): the margin that leaves about half the negatives
    active); batches of 3,000 / 0 / 2,500 (not a multiple of 8) / 64.  Every batch holds positives of mixed sides and an entry that is
    no corruption of its positive (make_batches).  single: the first batch carries ONE relation; many: 12,000 relations for at most
    3,000 positives, so that nearly every wave of a workgroup holds a relation of its own; two: 2 relations."""
    def with_mode(c, mode):
        c["rel_mode"] = mode
        return c
    return [sp.case("d36-k10", d=36, k=10, seed=36),
            sp.case("d75-k5-L1", d=75, k=5, norm="L1", neg_margin=12.0, seed=75),
            sp.case("d100-k10", d=100, k=10, seed=1100),
            sp.case("d100-k10-L1", d=100, k=10, norm="L1", neg_margin=13.8, seed=101),
            sp.case("d200-k5", d=200, k=5, seed=200),
            sp.case("d200-k10-L1", d=200, k=10, norm="L1", neg_margin=19.5, seed=201),
            with_mode(sp.case("d100-k10-single", d=100, k=10, n_rel=3, seed=102), "single"),
            with_mode(sp.case("d75-k5-single", d=75, k=5, n_rel=2, seed=103), "single"),
            sp.case("d100-k10-many", d=100, k=10, n_rel=12000, seed=104),
            sp.case("d36-k5-many", d=36, k=5, n_rel=12000, seed=105),
            sp.case("d100-k10-two", d=100, k=10, n_rel=2, seed=106)]


@pytest.mark.parametrize("env", ["order", "order-block256"])
def test_small_shapes_under_the_forced_plan(env, tmp_path, capsys):
    """teacher-forced against the oracle in a process under OEA_STEP_PLAN=2 (the plan whatever the table size).  order-block256:
    OEA_STEP_WAVE_BLOCK=256, workgroups of 4 waves that take two slots each -- every pass of the loop sums its own 4 rows."""
    cases = small_cases()
    extra = dict(OEA_STEP_PLAN="2", OEA_STEP_REL_ORDER="1")
    if env == "order-block256":
        extra["OEA_STEP_WAVE_BLOCK"] = "256"
    with capsys.disabled():
        print()
        out, factory = sp.run_worker(tmp_path, "rel-" + env, extra, cases)
        for ci, c in enumerate(cases):
            assert bool(out["%d_supported" % ci]), c["name"]
            pos, _, offsets = make_batches(c)
            first = pos[:int(offsets[1]), 1]
            if c.get("rel_mode") == "single":
                assert len(np.unique(first)) == 1
            if c["n_rel"] == 12000:
                assert len(np.unique(first)) > 0.75 * len(first) and c["n_rel"] > len(first)
            sp.check_case("%s %s" % (env, c["name"]), c, factory(ci), ("outside", "listed", "hubs"))


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the switch
# ---------------------------------------------------------------------------------------------------------------------------------


def free_cases():
    return [sp.case("free-d%d" % d, d=d, k=10, n_rel=n_rel, sizes=(3000, 0, 2500, 64, 2999), seed=700 + d)
            for d, n_rel in ((36, 200), (100, 40), (200, 5000))]


def free_worker():
    """three free-running epochs of every case (the plan is built in the first call of an epoch and found by the second)"""
    from openea_amd import ops
    ops.lib()
    out = {}
    for c in free_cases():
        pos, neg, offsets = make_batches(c)
        run = sp.DeviceRun(ops, c, pos, neg, offsets, sp.make_tables(c))
        assert run.supported
        loss = 0.0
        for _ in range(3):
            for lo, hi in ((0, 2), (2, len(c["sizes"]))):
                state, l, pad_ok, ws_ok = run.run(lo, hi)
                assert pad_ok and ws_ok
                loss += l
        out["e_" + c["name"]], out["r_" + c["name"]], out["l_" + c["name"]] = state[0], state[2], np.float64(loss)
    np.savez(os.environ["OEA_OUT"], **out)


def test_switch_off_equals_the_default(tmp_path):
    """OEA_STEP_REL_ORDER=0 (batch order, every wave its own relation row: the path before the order) against the default, both
    under OEA_STEP_PLAN=2: 15 free-running steps.  The two differ in the ORDER of fp32 additions into the relation scratch and of the
    loss partials only: tables within 2e-6 of their norm, loss within 1e-6 (the bounds of
    test_kernels_gpu.py::test_planned_epochs_equal_the_atomic_epochs)."""
    res = {}
    for sw in ("1", "0"):
        out = str(tmp_path / ("free%s.npz" % sw))
        run_script(dict(OEA_REL_MODE="free", OEA_OUT=out, OEA_STEP_PLAN="2", OEA_STEP_REL_ORDER=sw))
        res[sw] = dict(np.load(out))
    for c in free_cases():
        for t in ("e_", "r_"):
            a, b = res["0"][t + c["name"]], res["1"][t + c["name"]]
            err = np.linalg.norm(a - b) / np.linalg.norm(a)
            print("%s %s: |off - on| / |off| = %.3g" % (c["name"], t, err))
            assert err <= 2e-6, (c["name"], t, err)
        la, lb = float(res["0"]["l_" + c["name"]]), float(res["1"]["l_" + c["name"]])
        assert abs(la - lb) <= 1e-6 * abs(la), (c["name"], la, lb)
