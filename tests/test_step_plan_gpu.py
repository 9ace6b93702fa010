"""The PLANNED translational step against the C oracle, in every dispatch.

What runs: `triple_wave<..., PLAN = true>` (a positive's two gradient rows leave as plain stores into `contrib`) and the optimiser
of a planned step, `apply_step_plan<16, IT, true>` / `apply_step_plan<16, IT, false>` / `apply_step_plan<G, IT, false>` (sums `contrib` rows in
the plan's order, adds the atomic scratch where a row's touched flag is up, scans the flags for rows the plan does not list,
updates the relation rows, adds the loss partials), driven through the C ABI as the epoch engine drives them
(`ops.triple_epoch` with presampled negatives and a plan buffer), on negatives made HERE.  The other side is
`oracle.cport.triple_step` (C, double accumulation) on the same batches.

Per step, teacher-forced: step s runs on the device and in the oracle, the two are compared, then the oracle's tables and
accumulators are copied over the device's.  The workspace, `contrib` and the plan are NOT reset in between: stale scratch shows.
  * rows of both tables: `_tol.assert_rows_close` at the project's 1e-4;
  * accumulators `rtol 2e-3, atol 1e-6`, loss 1e-5 relative (as `test_fullsize_gpu.py::test_step_100k_shape`);
  * rows (tables and accumulators) that no triple of the step names: the same bits as before the step; pad columns stay zero;
  * the atomic scratch and the touched flags: all zero after the step.

Rows left out.  A triple whose float64 score is within 1e-5 of its margin may be active on one side and not on the other (an fp32
score differs from the float64 one by up to 1.5e-6 on these inputs; 1e-5 is 7 times that): the rows it names are left out of
that step's row and accumulator comparison (they still count for everything else).  At most 0.1 % of the entity rows a step
names and 3 % of its relation rows may be left out; above that the test fails.  Both counts are printed.

Branch counts.  For every step the test counts, in numpy from the oracle's state before the step: positives outside the plan's
rule, rows the plan lists, hub rows (more than 8 references), listed rows whose touched flag is up (the merge branch) and flagged
rows the plan does not list (the flag scan); it prints them and asserts they are above zero where a case is meant to cover them.

Run to run.  `test_planned_rows_keep_their_bits_run_to_run` needs no oracle: with no negative active, the rows whose whole gradient is
the plan's gathered sum must have the same bits when a step is repeated from the same state.
"""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HUB_ENTRIES = 8                  # csrc/step_plan.h: kPlanHubEntries
NEAR = 1e-5                      # |float64 score - margin| <= NEAR: the triple's rows are left out of the step's row comparison
PLAN_BLOCKS, SCAN_BLOCKS, MAX_PARTIALS = 8192, 4096, 4096      # csrc/triple_step.hip:launch_step's caps, csrc/step_rows.h:kMaxBlocks


@pytest.fixture(scope="module")
def ops():
    from openea_amd import ops as _ops
    _ops.lib()   # raises loudly if the HIP library / GPU is missing
    return _ops


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs: ONE seeded generator
# ---------------------------------------------------------------------------------------------------------------------------------


def case(name, n_ent=6000, n_rel=200, d=75, sizes=(3000, 0, 2500, 64), k=5, norm="L2", opt="Adagrad", neg_margin=3.0, pos_margin=0.01,
         seed=1, uniform=False, calls=None, repeat=False):
    """calls: None = every step in a call of its own, teacher-forced; a list of (lo, hi) = those ranges, free-running.
    repeat: no oracle -- every step twice from the same device state (worker_repeat)"""
    return dict(name=name, n_ent=n_ent, n_rel=n_rel, d=d, sizes=list(sizes), k=k, norm=norm, opt=opt, neg_margin=neg_margin,
                pos_margin=pos_margin, seed=seed, uniform=uniform, calls=calls, repeat=repeat)


def make_batches(c):
    """-> pos_all int32 [N, 3], neg_all int32 [N k, 3], offsets int64 [steps + 1].  Heads from a Zipf law (1 / rank^0.9), tails and
    relations uniform; a positive's k negatives all on ONE side (the sampler's output), 3 % of the positives with a side per
    negative; the corrupting entities from the same Zipf law, so that active negatives fall on rows the plan lists.
    uniform: heads and tails DISTINCT rows while the table lasts (no hubs: every row is a plan row), corrupting entities uniform.
    Planted in every batch: a negative that is no corruption of its positive; in the first: a self-loop, a negative equal to its
    positive, and the table's last two rows -- used by nothing else -- with exactly 8 and exactly 9 references (the hub threshold)."""
    rng = np.random.RandomState(c["seed"])
    n_ent, n_rel, k = c["n_ent"], c["n_rel"], c["k"]
    offsets = np.concatenate([[0], np.cumsum(c["sizes"])]).astype(np.int64)
    n, m = int(offsets[-1]), n_ent - 2                               # rows m, m + 1: the planted 8- and 9-reference rows
    w = 1.0 / np.arange(1, m + 1) ** 0.9
    w /= w.sum()
    if c["uniform"]:
        perm = np.concatenate([rng.permutation(m) for _ in range(-(-2 * n // m))])
        heads, tails = perm[:n], perm[n:2 * n]
    else:
        heads, tails = rng.choice(m, n, p=w), rng.randint(0, m, n)
    pos = np.stack([heads, rng.randint(0, n_rel, n), tails], 1).astype(np.int32)
    first = int(c["sizes"][0])
    assert first >= 64
    pos[3, 2] = pos[3, 0]                                            # a self-loop: both references on one row
    pos[10:18, 0] = m                                                # exactly 8 references: the last row the plan sums itself
    pos[20:29, 0] = m + 1                                            # exactly 9: the first hub
    side = rng.rand(n) < 0.5                                         # True: the head is corrupted
    mixed = rng.rand(n) < 0.03                                       # rounds after a collision: a side per negative
    mixed[:64] = False                                               # (the planted positives stay inside the plan's rule)
    mixed[40] = True                                                 # ... but for one
    side = np.where(np.repeat(mixed, k), rng.rand(n * k) < 0.5, np.repeat(side, k))
    ne = rng.randint(0, m, n * k) if c["uniform"] else rng.choice(m, n * k, p=w)
    neg = np.repeat(pos, k, 0)
    neg[side, 0] = ne[side]
    neg[~side, 2] = ne[~side]
    neg[5 * k] = pos[5]                                              # a negative equal to its positive (max_try exhausted)
    for b0, size in zip(offsets[:-1], c["sizes"]):
        if size >= 64:
            neg[(int(b0) + 7) * k] = (3, 1, 4)                       # an entry that is NOT a corruption of its positive (every batch: with
                                                                     # k = 1 nothing else puts a positive outside the plan's rule)
    return pos, neg.astype(np.int32), offsets


def make_tables(c):
    """tables standard_normal / sqrt(d), accumulators 0.1"""
    rng = np.random.RandomState(1000 + c["seed"])
    d = c["d"]
    ent = (rng.standard_normal((c["n_ent"], d)) / np.sqrt(d)).astype(np.float32)
    rel = (rng.standard_normal((c["n_rel"], d)) / np.sqrt(d)).astype(np.float32)
    return [ent, np.full_like(ent, 0.1), rel, np.full_like(rel, 0.1)]


def step_kw(c):
    return dict(loss="limited", loss_norm=c["norm"], pos_margin=c["pos_margin"], neg_margin=c["neg_margin"], balance=0.2,
                optimizer=c["opt"], lr=0.01)


def calls_of(c):
    return [tuple(x) for x in c["calls"]] if c["calls"] else [(s, s + 1) for s in range(len(c["sizes"]))]


# ---------------------------------------------------------------------------------------------------------------------------------
# the device side (in this process for the default dispatch, in a worker process per set of switches: they are read once)
# ---------------------------------------------------------------------------------------------------------------------------------


class DeviceRun:
    """raw tensors as the epoch engine holds them: tables, accumulators, workspace, plan buffer, the epoch's negatives"""

    def __init__(self, ops, c, pos, neg, offsets, state):
        import torch
        self.ops, self.torch, self.c, self.d = ops, torch, c, c["d"]
        self.ld = ops.pad4(self.d)
        self.e, self.ea, self.r, self.ra = (ops.to_table(a) for a in state)
        self.ea[:, self.d:] = 0.1                                     # (the accumulators' pad columns: 0.1 like the rest, never read back)
        self.ra[:, self.d:] = 0.1
        self.cfg = ops.make_step_cfg(neg_group_k=c["k"], **step_kw(c))
        self.ws = ops.step_workspace(c["n_ent"], c["n_rel"], self.ld)
        self.offsets = np.ascontiguousarray(offsets, np.int64)
        self.splits = np.ascontiguousarray(np.diff(self.offsets) // 2, np.int64)
        dev = self.e.device
        self.off_dev, self.spl_dev = torch.from_numpy(self.offsets).to(dev), torch.from_numpy(self.splits).to(dev)
        self.pos, self.neg = ops.to_ids(pos), ops.to_ids(neg)
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)
        self.loss = torch.zeros(1, dtype=torch.float64, device=dev)
        steps = len(self.splits)
        dims = (len(pos), steps, int(np.diff(self.offsets).max()), c["n_ent"], self.ld)
        self.plan = ops.step_plan_buffer(*dims, dev=dev)
        # the plan buffer is uninitialised memory that epochs reuse; fresh device memory happens to be zeros, which would hide a
        # `contrib` row that is summed without having been stored in this step: NaN in the whole `contrib` region stands for what
        # an earlier epoch left there (the build never writes it; triple_wave stores every row the plan lists)
        off = (C.c_int64 * 9)()
        ops.check(ops.lib().oea_step_plan_offsets(*dims, C.cast(off, C.c_void_p)))
        self.plan[off[5]: off[5] + 4 * 2 * max(dims[2], 1) * self.ld].view(torch.float32).fill_(float("nan"))
        self.built = False
        self.supported = ops.step_plan_supported(self.cfg, c["n_ent"], c["n_rel"], self.ld, c["k"])

    def set_state(self, state):
        for t, a in zip((self.e, self.ea, self.r, self.ra), state):
            t[:, :self.d].copy_(self.torch.from_numpy(a))

    def run(self, lo, hi):
        """steps [lo, hi) by one call -> (state, loss, pad columns still zero, scratch and flags all zero)"""
        torch, ops = self.torch, self.ops
        self.loss.zero_()
        ops.triple_epoch(self.e, self.ea, self.r, self.ra, self.d, self.pos, self.offsets, self.splits, self.c["k"], None, None, 0, 0,
                         self.neg, self.err, self.cfg, self.ws, self.loss, offsets_dev=self.off_dev, splits_dev=self.spl_dev,
                         step_range=(lo, hi), plan=(self.plan, self.built))
        self.built = True
        torch.cuda.synchronize()
        state = [t[:, :self.d].cpu().numpy() for t in (self.e, self.ea, self.r, self.ra)]
        pad_ok = not bool((self.e[:, self.d:] != 0).any().item()) and not bool((self.r[:, self.d:] != 0).any().item())
        ws_ok = not bool((self.ws[: self.ws.numel() - 8 * MAX_PARTIALS] != 0).any().item())     # (the loss partials are the tail)
        return state, float(self.loss.item()), pad_ok, ws_ok


def worker_main():
    """a worker process: the cases of OEA_IN (json + the oracle's states to force) on the device -> OEA_OUT"""
    from openea_amd import ops
    ops.lib()
    inp = np.load(os.environ["OEA_IN"])
    out = {}
    for ci, c in enumerate(json.loads(str(inp["cases"]))):
        pos, neg, offsets = make_batches(c)
        run = DeviceRun(ops, c, pos, neg, offsets, make_tables(c))
        out["%d_supported" % ci] = run.supported
        if c["repeat"]:
            worker_repeat(run, ci, c, out)
            continue
        for j, (lo, hi) in enumerate(calls_of(c)):
            if c["calls"] is None and j > 0:
                run.set_state([inp["%d_%d_%d" % (ci, j - 1, a)] for a in range(4)])
            state, loss, pad_ok, ws_ok = run.run(lo, hi)
            for a in range(4):
                out["%d_%d_%d" % (ci, j, a)] = state[a]
            out["%d_%d_misc" % (ci, j)] = np.array([loss, pad_ok, ws_ok], np.float64)
        del run
    np.savez(os.environ["OEA_OUT"], **out)


def worker_repeat(run, ci, c, out):
    """every step of a repeat case TWICE from the same tables, accumulators, workspace, plan and `contrib` (the plan buffer holds both).
    A first call builds the plan and is thrown away.  Every step starts from the case's initial tables: the same in every process.
    -> "<ci>_<s>_<a>p": array a before the step, "..._<a>": after the first run, "..._<a>b": after the second"""
    before = [t[:, :run.d].cpu().numpy() for t in (run.e, run.ea, run.r, run.ra)]
    run.run(0, 1)
    for s in range(len(c["sizes"])):
        run.set_state(before)
        ws0, plan0 = run.ws.clone(), run.plan.clone()
        first = run.run(s, s + 1)
        run.set_state(before)
        run.ws.copy_(ws0)
        run.plan.copy_(plan0)
        second = run.run(s, s + 1)
        for a in range(4):
            out["%d_%d_%dp" % (ci, s, a)], out["%d_%d_%d" % (ci, s, a)], out["%d_%d_%db" % (ci, s, a)] = before[a], first[0][a], second[0][a]
        out["%d_%d_misc" % (ci, s)] = np.array([first[1], first[2], first[3], second[1], second[2], second[3]], np.float64)


WORKER = r'''
import os, sys
sys.path[:0] = [os.environ["OEA_ROOT"], os.path.join(os.environ["OEA_ROOT"], "tests")]
import test_step_plan_gpu
test_step_plan_gpu.worker_main()
'''


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference side: the oracle's step, and the float64 restatement that counts the branches and finds the boundary triples
# ---------------------------------------------------------------------------------------------------------------------------------


def _scores64(ent, rel, tri, l1):
    """float64 scores of triples on l2-normalised rows (oracle.c:norm_row: v / sqrt(max(sum v^2, 1e-12)))"""
    out = np.empty(len(tri))
    for a in range(0, len(tri), 1 << 16):
        t = tri[a:a + (1 << 16)]
        rows = []
        for tab, ids in ((ent, t[:, 0]), (rel, t[:, 1]), (ent, t[:, 2])):
            v = tab[ids].astype(np.float64)
            rows.append(v / np.sqrt(np.maximum((v * v).sum(1, keepdims=True), 1e-12)))
        dd = rows[0] + rows[1] - rows[2]
        out[a:a + (1 << 16)] = np.abs(dd).sum(1) if l1 else (dd * dd).sum(1)
    return out


def step_facts(c, state, pos, neg):
    """what a step on `state` does, from float64 scores: the branch counts of the planned step (a restatement of step_plan.h and of
    triple_wave's use of it), the rows the step names, and the rows of triples within NEAR of their margin"""
    n_ent, n_rel, k, n = c["n_ent"], c["n_rel"], c["k"], len(pos)
    ent, rel = state[0], state[2]
    l1 = c["norm"] == "L1"
    pm, nm = float(np.float32(c["pos_margin"])), float(np.float32(c["neg_margin"]))    # the cfg holds floats
    sp, sn = _scores64(ent, rel, pos, l1), _scores64(ent, rel, neg, l1).reshape(n, k)
    act_p, act_n = sp > pm, sn < nm
    ng = neg.reshape(n, k, 3).astype(np.int64)
    p64 = pos.astype(np.int64)
    near_p, near_n = np.abs(sp - pm) <= NEAR, (np.abs(sn - nm) <= NEAR)
    skip_ent = np.unique(np.concatenate([p64[near_p][:, [0, 2]].ravel(), ng[near_n][:, [0, 2]].ravel()]))
    skip_rel = np.unique(np.concatenate([p64[near_p][:, 1], ng[near_n][:, 1]]))
    named_ent = np.zeros(n_ent, bool)
    named_ent[np.concatenate([p64[:, 0], p64[:, 2], ng[:, :, 0].ravel(), ng[:, :, 2].ravel()])] = True
    named_rel = np.zeros(n_rel, bool)
    named_rel[np.concatenate([p64[:, 1], ng[:, :, 1].ravel()])] = True
    # the plan's rule: every entry a corruption of its positive, all on one side
    same_h, same_t, same_r = ng[:, :, 0] == p64[:, :1], ng[:, :, 2] == p64[:, 2:], ng[:, :, 1] == p64[:, 1:2]
    inrule = (same_r & (same_h | same_t)).all(1) & (same_h.all(1) | same_t.all(1))
    tails = same_h.all(1)                                            # the negatives keep the head: tail side
    refs = np.bincount(np.concatenate([p64[inrule, 0], p64[inrule, 2]]), minlength=n_ent)
    listed, hub = (refs > 0) & (refs <= HUB_ENTRIES), refs > HUB_ENTRIES
    # rows that receive gradient through the atomic scratch (touched flag up): the corrupted rows of active negatives, ...
    flagged = np.zeros(n_ent, bool)
    ce = np.where(tails[:, None], ng[:, :, 2], ng[:, :, 0])
    flagged[ce[inrule[:, None] & act_n]] = True
    # ... a positive's own row where it is a hub of the step (the row that takes the whole sum moves with any active triple) ...
    anyact = act_p | act_n.any(1)
    flagged[p64[inrule & hub[p64[:, 0]] & np.where(tails, anyact, act_p), 0]] = True
    flagged[p64[inrule & hub[p64[:, 2]] & np.where(tails, act_p, anyact), 2]] = True
    # ... and both rows of every active triple of a positive outside the rule
    flagged[p64[~inrule & act_p][:, [0, 2]].ravel()] = True
    flagged[ng[~inrule[:, None] & act_n][:, [0, 2]].ravel()] = True
    counts = dict(outside=int((~inrule).sum()), listed=int(listed.sum()), hubs=int(hub.sum()), merge=int((listed & flagged).sum()),
                  scan=int((flagged & ~listed).sum()), max_refs=int(refs.max()) if n else 0,
                  active_neg=float(act_n.mean()) if n else 0.0, active_pos=float(act_p.mean()) if n else 0.0)
    scan_rows = np.nonzero(flagged & ~listed)[0]
    return dict(counts=counts, named_ent=named_ent, named_rel=named_rel, skip_ent=skip_ent, skip_rel=skip_rel, refs=refs,
                scan_rows=scan_rows, near=int(near_p.sum() + near_n.sum()))


_TRAJ = {}


def oracle_steps(c, pos, neg, offsets, tables=None):
    """the oracle's trajectory, free-running (teacher-forcing the device towards it does not change it):
    -> [(s, state before, state after, loss, facts)] per step (kept for the small tables: a worker's input and the check share it)"""
    from oracle import cport
    key = json.dumps(c, sort_keys=True)
    if key in _TRAJ:
        return _TRAJ[key]
    state, traj = tables if tables is not None else make_tables(c), []
    for s in range(len(c["sizes"])):
        lo, hi = int(offsets[s]), int(offsets[s + 1])
        before = state
        state = [a.copy() for a in before]
        p, g = pos[lo:hi], neg[lo * c["k"]: hi * c["k"]]
        facts = step_facts(c, before, p, g)
        loss = cport.triple_step(state[0], state[1], state[2], state[3], p, g, **step_kw(c)) if hi > lo else 0.0
        traj.append((s, before, state, float(loss), facts))
    if c["n_ent"] * c["d"] <= 10000000:
        _TRAJ[key] = traj
    return traj


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def compare(tag, c, before, got, ref, loss_got, loss_ref, pad_ok, ws_ok, named_ent, named_rel, skip_ent, skip_rel, caps=(0.001, 0.03)):
    """the assertions of one call.  before: what the device started the call from"""
    from _tol import assert_rows_close
    n_named_e, n_named_r = int(named_ent.sum()), int(named_rel.sum())
    print("%s: rows left out (a triple within %.0e of its margin): %d of %d named entity rows, %d of %d named relation rows"
          % (tag, NEAR, len(skip_ent), n_named_e, len(skip_rel), n_named_r))
    assert len(skip_ent) <= caps[0] * n_named_e and len(skip_rel) <= caps[1] * n_named_r, "%s: too many rows left out" % tag
    keep_e, keep_r = np.ones(len(ref[0]), bool), np.ones(len(ref[2]), bool)
    keep_e[skip_ent] = False
    keep_r[skip_rel] = False
    assert_rows_close(got[0][keep_e], ref[0][keep_e], tag + ", entity table")
    assert_rows_close(got[2][keep_r], ref[2][keep_r], tag + ", relation table")
    np.testing.assert_allclose(got[1][keep_e], ref[1][keep_e], rtol=2e-3, atol=1e-6, err_msg=tag + ", entity accumulators")
    np.testing.assert_allclose(got[3][keep_r], ref[3][keep_r], rtol=2e-3, atol=1e-6, err_msg=tag + ", relation accumulators")
    print("%s: loss %.6f (oracle %.6f)" % (tag, loss_got, loss_ref))
    assert abs(loss_got - loss_ref) <= 1e-5 * abs(loss_ref), "%s: loss %.9g, oracle %.9g" % (tag, loss_got, loss_ref)
    for a, named, what in ((0, named_ent, "entity rows"), (1, named_ent, "entity accumulators"), (2, named_rel, "relation rows"),
                           (3, named_rel, "relation accumulators")):
        assert _same_bits(got[a][~named], before[a][~named]), "%s: %s that no triple names moved" % (tag, what)
    assert pad_ok, "%s: pad columns of a table are not zero" % tag
    assert ws_ok, "%s: atomic scratch / touched flags not all zero after the step" % tag


def check_case(tag, c, run_call, expect, tables=None):
    """one case: the oracle step by step, the device through run_call(j, lo, hi, forced state or None) -> DeviceRun.run's tuple.
    expect: names of the branch counts that must be above zero in every full batch.  -> the per-step counts"""
    pos, neg, offsets = make_batches(c)
    traj = oracle_steps(c, pos, neg, offsets, tables)
    all_counts = []
    for s, _, _, _, facts in traj:
        if c["sizes"][s]:
            print("%s step %d: %s" % (tag, s, facts["counts"]))
            for key in expect if c["sizes"][s] >= 1000 else ("outside", "listed"):    # (the batch of 64 is there for its size: no hub)
                assert facts["counts"][key] > 0, "%s step %d does not reach the '%s' branch" % (tag, s, key)
            all_counts.append(facts["counts"])
    m = c["n_ent"] - 2                                               # the planted rows: 8 references = listed, 9 = the first hub
    assert traj[0][4]["refs"][m] == HUB_ENTRIES and traj[0][4]["refs"][m + 1] == HUB_ENTRIES + 1
    dev_before = traj[0][1]                                          # the initial tables
    for j, (lo, hi) in enumerate(calls_of(c)):
        forced = None
        if c["calls"] is None:                                       # teacher-forced: the device starts from the oracle's state
            forced = traj[lo][1] if j > 0 else None
            dev_before = traj[lo][1]
        got, loss, pad_ok, ws_ok = run_call(j, lo, hi, forced)
        steps = traj[lo:hi]
        named_ent = np.logical_or.reduce([f["named_ent"] for *_, f in steps])
        named_rel = np.logical_or.reduce([f["named_rel"] for *_, f in steps])
        skip_ent = np.unique(np.concatenate([f["skip_ent"] for *_, f in steps]))
        skip_rel = np.unique(np.concatenate([f["skip_rel"] for *_, f in steps]))
        caps = (0.001, 0.03) if hi - lo == 1 else (0.003, 0.06)
        compare("%s steps [%d, %d)" % (tag, lo, hi), c, dev_before, got, steps[-1][2], loss, sum(x[3] for x in steps), pad_ok, ws_ok,
                named_ent, named_rel, skip_ent, skip_rel, caps)
        dev_before = got
    return all_counts, traj


_WORKERS = {}


def run_worker(tmp_path, tag, env_extra, cases):
    """the cases on the device in ONE fresh process under env_extra -> run_call factory for check_case.  Teacher forcing needs the
    oracle's states before the worker starts: they are computed here and handed over in the .npz."""
    if tag in _WORKERS:                                              # (the tests that share a set of switches share its process)
        return _WORKERS[tag]
    inp = {"cases": np.array(json.dumps(cases))}
    for ci, c in enumerate(cases):
        if c["calls"] is None and not c["repeat"]:
            pos, neg, offsets = make_batches(c)
            for s, _, after, _, _ in oracle_steps(c, pos, neg, offsets)[:-1]:      # (nothing starts from the last step's state)
                for a in range(4):
                    inp["%d_%d_%d" % (ci, s, a)] = after[a]
    fin, fout = str(tmp_path / ("in_%s.npz" % tag)), str(tmp_path / ("out_%s.npz" % tag))
    np.savez(fin, **inp)
    env = dict(os.environ, OEA_ROOT=ROOT, OEA_IN=fin, OEA_OUT=fout)
    for key in ("OEA_STEP_DETERMINISTIC", "OEA_STEP_WAVE", "OEA_STEP_PLAN", "OEA_APPLY_G16", "OEA_APPLY_V4", "OEA_STEP_RUNTIME_KIND"):
        env.pop(key, None)                                           # only the switches this worker is about
    env.update(env_extra)
    t0 = time.time()
    p = subprocess.run([sys.executable, "-c", WORKER], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert p.returncode == 0, p.stdout.decode(errors="replace")[-3000:]
    print("worker %s %s: %d cases in %.1f s" % (tag, env_extra, len(cases), time.time() - t0))
    out = np.load(fout)

    def factory(ci):
        def run_call(j, lo, hi, forced):
            misc = out["%d_%d_misc" % (ci, j)]
            return [out["%d_%d_%d" % (ci, j, a)] for a in range(4)], float(misc[0]), bool(misc[1]), bool(misc[2])
        return run_call
    _WORKERS[tag] = (out, factory)
    return out, factory


# ---------------------------------------------------------------------------------------------------------------------------------
# case 1: the default dispatch at size
# ---------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("neg_margin", [2.0, 3.0])
def test_default_dispatch_at_the_100k_shape(ops, neg_margin, capsys):
    """EN-FR-100K shape (200,000 entities, 700 relations, d 100, three batches of 20,000, k 10), no switch set: tables + state of
    241 MB make the library choose the plan, 16-lane groups and float4 rows (`triple_wave<2, 0, 10, true>`,
    `apply_step_plan<16, 7, true>`).  Three teacher-forced Adagrad steps.  neg_margin 2.0: few negatives are active (the merge branch
    and the flag scan see a few hundred rows); 3.0: about half of them are (thousands of rows in both)."""
    c = case("100k", n_ent=200000, n_rel=700, d=100, sizes=(20000, 20000, 20000), k=10, neg_margin=neg_margin, seed=7)
    pos, neg, offsets = make_batches(c)
    tables = make_tables(c)
    run = DeviceRun(ops, c, pos, neg, offsets, tables)
    assert run.supported, "the default dispatch does not choose the plan at the 100K shape"

    def run_call(j, lo, hi, forced):
        if forced is not None:
            run.set_state(forced)
        return run.run(lo, hi)
    with capsys.disabled():
        print()
        check_case("100K shape, neg_margin %.1f" % neg_margin, c, run_call, ("outside", "listed", "hubs", "merge", "scan"), tables)


# ---------------------------------------------------------------------------------------------------------------------------------
# cases 2 and 3: every instance at a small shape, and the grid-stride edges, one process per set of switches
# ---------------------------------------------------------------------------------------------------------------------------------


def small_cases():
    """every value of every axis at least once: d (ld 24, 52, 76, 96, 100, 128, 200 = 2, 4, 5, 6, 7, 8 fragments of 16 lanes and the
    64-lane kernel) with Adagrad, L2, k 10 (the KT = 10 instance of triple_wave); k 5 and 1 (KT = 0); L1; SGD; neg_margin 2.0 once;
    pos_margin 3.0 once (many positives inactive: their contrib rows are still stored and summed, and must be zeros).  Not the full
    product: the last three cases carry two axes each, to keep the file's wall time at that of test_kernels_gpu.py"""
    # (seeds: at seed 100 the ORACLE alone has three triples within NEAR of a margin in one step of d = 100: 6 of 5,355 named entity
    #  rows, above the 0.1 % a step may leave out -- a property of the inputs, so that case takes another seed)
    cs = [case("d%d" % d, d=d, k=10, seed=d if d != 100 else 1100) for d in (24, 50, 75, 96, 100, 128, 200)]
    # (an L1 score of unit rows is about 1.4 sqrt(d): the margin that leaves half the negatives active is 12 at d = 75, 15.5 at 128;
    #  at 3.0 no negative would be active and the L1 cases would not reach the merge branch)
    cs += [case("d75-k5-L1", d=75, k=5, norm="L1", neg_margin=12.0, seed=301),
           case("d100-k1-sgd-nm2-pm3", d=100, k=1, opt="SGD", neg_margin=2.0, pos_margin=3.0, seed=302),
           case("d128-k10-L1-sgd", d=128, k=10, norm="L1", opt="SGD", neg_margin=15.5, seed=303)]
    return cs


def edge_cases():
    return [
        # one batch of 70,000 positives on distinct rows: 140,000 plan rows > PLAN_BLOCKS * 16 lane groups (* 8 with 32-lane groups):
        # the plan part's grid stride; 70,000 / 8 = 8,750 workgroups' worth of loss partials > kMaxBlocks: the scoring kernel's
        case("stride-plan", n_ent=300000, n_rel=200, d=32, sizes=(70000,), k=1, seed=401, uniform=True),
        # 1,200,000 rows = 18,750 chunks of 64 flags > SCAN_BLOCKS * 4 waves: the flag scan's grid stride
        case("stride-scan", n_ent=1200000, n_rel=200, d=8, sizes=(5000,), k=5, seed=402, uniform=True),
    ]


ENVS = {"g0": dict(OEA_STEP_PLAN="2", OEA_APPLY_G16="0"),
        "g16": dict(OEA_STEP_PLAN="2", OEA_APPLY_G16="1"),
        "g16-dword": dict(OEA_STEP_PLAN="2", OEA_APPLY_G16="1", OEA_APPLY_V4="0"),
        # the plan refused: the flag-driven optimiser with 16-lane groups (`apply_rows<16, 2|4|5|6|7|8>`; d 200: `apply_rows<64, 4>`)
        "atomic-g16": dict(OEA_STEP_PLAN="0", OEA_APPLY_G16="1")}


REPEAT_ENVS = ("g0", "g16", "g16-dword")


def repeat_cases():
    """test_planned_rows_keep_their_bits_run_to_run: one batch of 3,000 and one of 64 (the batch's last workgroup), k 5, and
    neg_margin 0.0: the limited loss makes a negative active only when neg_margin - s > 0, and s >= 0, so NO negative is active and
    an entity row receives an atomic only as a hub or from a positive outside the plan's rule.  d 24: a float4 fragment that only
    lanes 0-5 fill; d 100: the second float4 fragment ends at lane 8, and the dword row has seven fragments; d 128: a full row;
    d 200: the 64-lane kernel -- the smallest shapes at which a fragment's bound or a lane group's tail can go wrong"""
    kw = dict(sizes=(3000, 64), k=5, pos_margin=0.01, neg_margin=0.0, repeat=True)
    return [case("repeat-d%d" % d, d=d, seed=700 + d, **kw) for d in (24, 100, 128, 200)] + \
           [case("repeat-d100-sgd", d=100, opt="SGD", seed=801, **kw)]


def env_cases(env):
    """what the worker process of a set of switches runs"""
    cs = small_cases() + (edge_cases() if env in ("g0", "g16") else [])
    if env in REPEAT_ENVS:
        cs += repeat_cases()
    if env == "g0":
        cs.append(case("ranges", d=75, k=5, neg_margin=2.0, seed=501, calls=[(0, 2), (2, 4)]))
    return cs


@pytest.mark.parametrize("env", sorted(ENVS))
def test_every_instance_and_the_grid_stride_edges(env, tmp_path, capsys):
    """OEA_STEP_PLAN=2 (the plan whatever the table size) with 32-lane groups (`apply_step_plan<32, 1..4, false>`, `<64, 4, false>`), 16-lane groups
    and float4 rows (`apply_step_plan<16, 2|4|5|6|7|8, true>`), 16-lane groups and dword fragments (`apply_step_plan<16, ..., false>`):
    small_cases() on 6,000 entities in batches of 3,000 / 0 (empty) / 2,500 / 64, teacher-forced; in the first two also
    edge_cases(), where a grid-stride loop of the optimiser kernel runs more than once.
    "atomic-g16": OEA_STEP_PLAN=0 with 16-lane groups -- no plan, every gradient through the atomic scratch and the flag-driven
    `apply_rows<16, 2|4|5|6|7|8>` (`<64, 4>` at d 200), held to the same oracle steps with the same checks and left-out caps."""
    cases = env_cases(env)
    with capsys.disabled():
        print()
        out, factory = run_worker(tmp_path, env, ENVS[env], cases)
        for ci, c in enumerate(cases):
            if c["calls"] is not None or c["repeat"]:                # test_step_ranges_across_calls, test_planned_rows_keep_...
                continue
            assert bool(out["%d_supported" % ci]) == (env != "atomic-g16"), c["name"]
            tag = "%s %s" % (env, c["name"])
            expect = ("outside", "listed", "hubs", "merge", "scan")
            if c["neg_margin"] == 2.0:
                expect = ("outside", "listed", "hubs")
            if env == "atomic-g16":
                expect = ()                                          # (no plan: none of its branches runs)
            counts, traj = check_case(tag, c, factory(ci), expect)
            if c["name"] == "stride-plan":
                groups = PLAN_BLOCKS * (16 if env != "g0" else 8)
                assert counts[0]["listed"] + counts[0]["hubs"] > groups and c["sizes"][0] // 8 > MAX_PARTIALS
            if c["name"] == "stride-scan":
                n_chunk = (c["n_ent"] + 63) // 64
                assert n_chunk > SCAN_BLOCKS * 4 and int((traj[0][4]["scan_rows"] % n_chunk >= SCAN_BLOCKS * 4).sum()) > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# case 4: step ranges across calls, free-running
# ---------------------------------------------------------------------------------------------------------------------------------


def test_step_ranges_across_calls(tmp_path, capsys):
    """steps [0, 2) by one call and [2, 4) by the next (the plan is built by the first and found by the second), free-running against
    the free-running oracle at neg_margin 2.0; the rows left out accumulate over the steps of a call (caps 0.3 % and 6 %).
    (In the process of the 32-lane switches: what OEA_STEP_PLAN=2 alone chooses at this size.)"""
    cases = env_cases("g0")
    with capsys.disabled():
        print()
        out, factory = run_worker(tmp_path, "g0", ENVS["g0"], cases)
        ci = len(cases) - 1
        assert cases[ci]["name"] == "ranges" and bool(out["%d_supported" % ci])
        check_case("ranges", cases[ci], factory(ci), ("outside", "listed", "hubs"))


# ---------------------------------------------------------------------------------------------------------------------------------
# case 5: the two predicates
# ---------------------------------------------------------------------------------------------------------------------------------


def test_plan_and_scoring_kernel_are_chosen_by_one_rule(tmp_path, capsys):
    """OEA_STEP_RUNTIME_KIND=1 sends the scoring to `triple_grouped`, which knows nothing of the plan (it neither stores `contrib` rows
    nor reads the hub flags).  Whether `step_plan_supported` then says yes or no, the step must equal the oracle.  Before the two
    decisions shared one rule it said yes: the optimiser added stale / uninitialised `contrib` rows on top of gradients that had
    all gone through the atomics -- with the NaN that DeviceRun leaves in `contrib`, every listed row came out NaN."""
    c = case("runtime-kind", d=75, k=5, seed=601)
    with capsys.disabled():
        print()
        out, factory = run_worker(tmp_path, "kind", dict(OEA_STEP_PLAN="2", OEA_STEP_RUNTIME_KIND="1"), [c])
        print("OEA_STEP_RUNTIME_KIND=1: step_plan_supported = %s" % bool(out["0_supported"]))
        check_case("runtime-kind", c, factory(0), ("outside", "listed", "hubs", "merge", "scan"))


# ---------------------------------------------------------------------------------------------------------------------------------
# case 6: rows summed from the plan have the same bits run to run
# ---------------------------------------------------------------------------------------------------------------------------------


def planned_only_rows(c, pos, neg):
    """of one step, in numpy from the batch -> (rows whose whole gradient is the plan's gathered sum when no negative is active: named
    as head or tail by positives inside the plan's rule only, at most HUB_ENTRIES times; rows the step's positives name; rows only its
    negatives name; every row it names).  Left out of the first: hubs, and every row a positive outside the rule or one of its
    negatives names (their gradients go through the atomic scratch)"""
    n_ent, k = c["n_ent"], c["k"]
    p64, ng = pos.astype(np.int64), neg.reshape(len(pos), k, 3).astype(np.int64)
    same_h, same_t, same_r = ng[:, :, 0] == p64[:, :1], ng[:, :, 2] == p64[:, 2:], ng[:, :, 1] == p64[:, 1:2]
    inrule = (same_r & (same_h | same_t)).all(1) & (same_h.all(1) | same_t.all(1))
    refs = np.bincount(np.concatenate([p64[inrule, 0], p64[inrule, 2]]), minlength=n_ent)
    outside = np.zeros(n_ent, bool)
    outside[p64[~inrule][:, [0, 2]].ravel()] = True
    outside[ng[~inrule][:, :, [0, 2]].ravel()] = True
    by_pos, by_neg = np.zeros(n_ent, bool), np.zeros(n_ent, bool)
    by_pos[p64[:, [0, 2]].ravel()] = True
    by_neg[ng[:, :, [0, 2]].ravel()] = True
    return (refs > 0) & (refs <= HUB_ENTRIES) & ~outside, by_pos, by_neg & ~by_pos, by_pos | by_neg


def check_repeat(env, cases, out):
    """the assertions of test_planned_rows_keep_their_bits_run_to_run on the output of a worker that ran `cases`"""
    seen = 0
    for ci, c in enumerate(cases):
        if not c["repeat"]:
            continue
        seen += 1
        assert bool(out["%d_supported" % ci]), c["name"]
        pos, neg, offsets = make_batches(c)
        n_keep = n_named = 0
        for s in range(len(c["sizes"])):
            lo, hi = int(offsets[s]), int(offsets[s + 1])
            keep, by_pos, only_neg, named = planned_only_rows(c, pos[lo:hi], neg[lo * c["k"]: hi * c["k"]])
            tag = "%s %s step %d" % (env, c["name"], s)
            before, first, second = ([out["%d_%d_%d%s" % (ci, s, a, sfx)] for a in range(2)] for sfx in ("p", "", "b"))
            misc = out["%d_%d_misc" % (ci, s)]
            assert misc[1] and misc[2] and misc[4] and misc[5], "%s: pad columns / scratch not clean after a run" % tag
            for got in (first, second):
                assert _same_bits(got[0][only_neg], before[0][only_neg]) and _same_bits(got[1][only_neg], before[1][only_neg]), \
                    "%s: a row that only negatives name moved: a negative was active" % tag
            moved = (first[0][keep] != before[0][keep]).any(1)
            print("%s: %d rows compared of %d the positives name (%d named in all, %d by negatives only); %d of them moved; "
                  "loss %.6f / %.6f" % (tag, keep.sum(), by_pos.sum(), named.sum(), only_neg.sum(), moved.sum(), misc[0], misc[3]))
            assert 2 * keep.sum() > by_pos.sum() and 2 * moved.sum() > keep.sum(), "%s: the compared set is too small" % tag
            assert _same_bits(first[0][keep], second[0][keep]), "%s: planned entity rows differ between two runs" % tag
            assert _same_bits(first[1][keep], second[1][keep]), "%s: planned accumulator rows differ between two runs" % tag
            n_keep, n_named = n_keep + int(keep.sum()), n_named + int(named.sum())
        assert 2 * n_keep > n_named, "%s %s: %d rows compared of %d named" % (env, c["name"], n_keep, n_named)
    assert seen == 5


@pytest.mark.parametrize("env", REPEAT_ENVS)
def test_planned_rows_keep_their_bits_run_to_run(env, tmp_path, capsys):
    """step_plan.h promises "no atomics, no order dependence" for the rows the plan sums.  repeat_cases() under the 32-lane, the
    16-lane float4 and the 16-lane dword switches: every step runs twice from the same tables, accumulators, workspace, `contrib` and
    plan (worker_repeat), and the entity rows and accumulator rows of planned_only_rows() must come out with the same BITS.  No
    oracle, no tolerance.  Relation rows and every other entity row are not compared: their sums go through atomics.
    That no negative was active is read from the device's own numbers: a row that only negatives name keeps its bits through the
    step (an active negative moves the row it corrupts).
    The compared set must be more than half of the rows the step's positives name, and over the case's two steps more than half of
    ALL the rows they name, negatives' included (2,884 of 5,062 at d 24; the batch of 64 alone cannot reach that: its 320
    negatives name about 210 rows that no positive names, against about 115 that its positives name), and most of it must move."""
    cases = env_cases(env)
    with capsys.disabled():
        print()
        out, _ = run_worker(tmp_path, env, ENVS[env], cases)
        check_repeat(env, cases, out)
