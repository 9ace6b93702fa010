"""Mixed-side positives in `triple_wave` against the C oracle.

The sampler finishes a positive whose first round collided in a second round with the other side's coin (batch.py:101-107), so a
few positives per step have head corruptions AND tail corruptions among their k negatives.  `triple_wave` scores those in the wave
(one round trip for the k corrupted rows, one wave-uniform branch per negative, the positive's rows through the atomic scratch)
instead of as 1 + k independent triples.  Here EVERY positive is such a positive: a coin per negative.

What runs: the per-step API (`ops.triple_step`: `triple_wave<..., PLAN = false>` + `apply_rows`) in this process, and the planned
epoch call (`ops.triple_epoch` with a plan buffer under OEA_STEP_PLAN=2: `triple_wave<..., PLAN = true>` with the relation order +
`apply_step_plan<G, IT, V4>`) in one worker process, as tests/test_step_plan_gpu.py does it.  The other side is `oracle.cport.triple_step`
(C, double accumulation) on the same batch.  Limits as in tests/test_step_plan_gpu.py: rows `_tol.assert_rows_close` at 1e-4,
accumulators rtol 2e-3 / atol 1e-6, loss 1e-5 relative, rows no triple names keep their bits, scratch and flags zero afterwards.

Inputs (seeded): 700 entities, 5 relations; heads and tails of the batch distinct rows; every other positive's tail row is set
close to l2n(h + r), so that positives INSIDE their margin occur and have active negatives; corrupting entities uniform.  Planted:
positive 0 has a negative equal to itself (it counts as a tail corruption) and all its other negatives but one on the tail side;
positive 2 (batches of 8 and 91) is a self-loop.  Nothing is left out of the comparison: `reference` asserts from float64 scores
that no triple lies within 1e-5 of its margin (an fp32 score differs from the float64 one by about 1e-6 on these inputs).

Margins: pos_margin 1.5, neg_margin 3.0 for the squared-L2 score (unrelated unit rows score about 3: both hinge states occur).  An
L1 score of the same rows is about 0.8 sqrt(3 d) (14 at d = 100): under those two numbers no L1 negative would be active, so the L1
cases keep the ratio and scale: neg_margin = the median float64 L1 score of the case's negatives rounded to a multiple of 0.5,
pos_margin = half of it.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import test_step_plan_gpu as sp

pytestmark = pytest.mark.gpu

ROOT = sp.ROOT
N_ENT, N_REL = 700, 5
BATCHES, DIMS, KS, NORMS = (91, 8, 1), (100, 128, 75, 200), (10, 3), ("L2", "L1")


@pytest.fixture(scope="module")
def ops():
    from openea_amd import ops as _ops
    _ops.lib()   # raises loudly if the HIP library / GPU is missing
    return _ops


def case(batch, d, k, norm, foreign=False):
    return dict(name="b%d-d%d-k%d-%s%s" % (batch, d, k, norm, "-foreign" if foreign else ""), n_ent=N_ENT, n_rel=N_REL, d=d,
                sizes=[batch], k=k, norm=norm, opt="Adagrad", pos_margin=1.5, neg_margin=3.0, seed=7000 + 13 * batch + d + 1000 * k,
                foreign=foreign)


def all_cases():
    cs = [case(b, d, k, n) for b in BATCHES for d in DIMS for k in KS for n in NORMS]
    return cs + [case(91, 100, 10, "L2", foreign=True)]


def make_inputs(c):
    """-> pos int32 [B, 3], neg int32 [B k, 3], state [ent, ent_acc, rel, rel_acc], c with the margins of its norm"""
    rng = np.random.RandomState(c["seed"])
    n, k, d = c["sizes"][0], c["k"], c["d"]
    rows = rng.permutation(N_ENT)[:2 * n]
    pos = np.stack([rows[:n], rng.randint(0, N_REL, n), rows[n:]], 1).astype(np.int32)
    if n > 2:
        pos[2, 2] = pos[2, 0]                                        # a self-loop
    ent = (rng.standard_normal((N_ENT, d)) / np.sqrt(d)).astype(np.float32)
    rel = (rng.standard_normal((N_REL, d)) / np.sqrt(d)).astype(np.float32)

    def l2n(v):
        return v / np.sqrt((v * v).sum())
    for p in range(0, n, 2):                                         # every other positive inside its margin: t ~ l2n(h + r)
        h, r, t = pos[p]
        if h != t:
            ent[t] = (l2n(l2n(ent[h].astype(np.float64)) + l2n(rel[r].astype(np.float64))) + 0.02 * rng.standard_normal(d)).astype(np.float32)
    head_side = rng.rand(n, k) < 0.5                                 # a coin per negative ...
    head_side[:, 0], head_side[:, 1] = False, True                   # ... and both sides in every positive
    head_side[0, 2:] = False                                         # positive 0: all but one on the tail side
    ne = rng.randint(0, N_ENT, (n, k))
    neg = np.repeat(pos, k, 0).reshape(n, k, 3)
    neg[:, :, 0] = np.where(head_side, ne, neg[:, :, 0])
    neg[:, :, 2] = np.where(head_side, neg[:, :, 2], ne)
    neg[0, 2] = pos[0]                                               # a negative equal to its positive (max_try exhausted)
    if c["foreign"]:
        neg[5, 4] = (pos[5, 0], (pos[5, 1] + 1) % N_REL, ne[5, 4])   # another relation: not a corruption of its positive
        neg[6, 3] = (ne[6, 3], pos[6, 1], ne[6, 4])                  # both entities differ
    neg = np.ascontiguousarray(neg.reshape(n * k, 3).astype(np.int32))
    c = dict(c)
    if c["norm"] == "L1":
        nm = float(np.round(2.0 * np.median(sp._scores64(ent, rel, neg, True))) / 2.0)      # (a multiple of 0.5: exact in fp32)
        c["neg_margin"], c["pos_margin"] = nm, 0.5 * nm
    return pos, neg, [ent, np.full_like(ent, 0.1), rel, np.full_like(rel, 0.1)], c


_REF = {}


def reference(c0):
    """the oracle's step, once per case: -> dict(c, pos, neg, before, after, loss, named_ent, named_rel)"""
    key = json.dumps(c0, sort_keys=True)
    if key in _REF:
        return _REF[key]
    from oracle import cport
    pos, neg, state, c = make_inputs(c0)
    n, k = len(pos), c["k"]
    l1 = c["norm"] == "L1"
    pm, nm = float(np.float32(c["pos_margin"])), float(np.float32(c["neg_margin"]))       # the cfg holds floats
    s_pos, s_neg = sp._scores64(state[0], state[2], pos, l1), sp._scores64(state[0], state[2], neg, l1).reshape(n, k)
    gap = min(float(np.abs(s_pos - pm).min()), float(np.abs(s_neg - nm).min()))
    assert gap > sp.NEAR, "%s: a triple within %.0e of its margin (%.3g): pick another seed" % (c["name"], sp.NEAR, gap)
    ng = neg.reshape(n, k, 3)
    same_h, same_t, same_r = ng[:, :, 0] == pos[:, :1], ng[:, :, 2] == pos[:, 2:], ng[:, :, 1] == pos[:, 1:2]
    foreign = ~(same_r & (same_h | same_t))
    mixed = ~foreign.any(1) & ~same_h.all(1) & ~same_t.all(1)
    assert int(foreign.any(1).sum()) == (2 if c["foreign"] else 0) and bool((mixed | foreign.any(1)).all()), c["name"]
    act_p, act_n = s_pos > pm, s_neg < nm
    facts = dict(mixed=int(mixed.sum()), active_pos=int(act_p.sum()), active_neg=int(act_n.sum()), negs=n * k,
                 inside_with_active=int((~act_p & act_n.any(1)).sum()), equal_to_pos=int((same_h & same_t & same_r).sum()),
                 self_loops=int((pos[:, 0] == pos[:, 2]).sum()), gap=gap)
    assert facts["equal_to_pos"] >= 1 and int((~same_h[0]).sum()) == 1, c["name"]
    if n >= 8:                                                       # both hinge states, and a positive inside its margin with active negatives
        assert 0 < facts["active_neg"] < n * k and 0 < facts["active_pos"] < n and facts["inside_with_active"] > 0, (c["name"], facts)
        assert facts["self_loops"] == 1
    after = [a.copy() for a in state]
    loss = float(cport.triple_step(after[0], after[1], after[2], after[3], pos, neg, **sp.step_kw(c)))
    named_ent, named_rel = np.zeros(N_ENT, bool), np.zeros(N_REL, bool)
    named_ent[np.concatenate([pos[:, 0], pos[:, 2], neg[:, 0], neg[:, 2]])] = True
    named_rel[np.concatenate([pos[:, 1], neg[:, 1]])] = True
    _REF[key] = dict(c=c, pos=pos, neg=neg, before=state, after=after, loss=loss, named_ent=named_ent, named_rel=named_rel, facts=facts)
    return _REF[key]


def check(tag, ref, got, loss, pad_ok, ws_ok):
    none = np.zeros(0, np.int64)
    print("%s: %s" % (tag, ref["facts"]))
    sp.compare(tag, ref["c"], ref["before"], got, ref["after"], loss, ref["loss"], pad_ok, ws_ok, ref["named_ent"], ref["named_rel"],
               none, none)


# ---------------------------------------------------------------------------------------------------------------------------------
# the per-step API: triple_wave<..., PLAN = false> + apply_rows
# ---------------------------------------------------------------------------------------------------------------------------------


def run_step(ops, ref):
    import torch
    c, d = ref["c"], ref["c"]["d"]
    e, ea, r, ra = (ops.to_table(a) for a in ref["before"])
    ea[:, d:] = 0.1
    ra[:, d:] = 0.1
    cfg = ops.make_step_cfg(neg_group_k=c["k"], **sp.step_kw(c))
    ws = ops.step_workspace(N_ENT, N_REL, e.shape[1])
    loss = torch.zeros(1, dtype=torch.float64, device=e.device)
    ops.triple_step(e, ea, r, ra, d, ops.to_ids(ref["pos"]), ops.to_ids(ref["neg"]), cfg, ws, loss)
    torch.cuda.synchronize()
    got = [t[:, :d].cpu().numpy() for t in (e, ea, r, ra)]
    pad_ok = not bool((e[:, d:] != 0).any().item()) and not bool((r[:, d:] != 0).any().item())
    ws_ok = not bool((ws[: ws.numel() - 8 * sp.MAX_PARTIALS] != 0).any().item())
    return got, float(loss.item()), pad_ok, ws_ok


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("batch", BATCHES)
def test_step_api(ops, batch, d, k, norm, capsys):
    """one step through `ops.triple_step`: 91 positives = 12 workgroups, the last with three waves past the end; 8 = one; 1 = one wave.
    d 100 / 75: a partial last fragment; 128: full fragments; 200: four fragments (`IT = 4`).  k 10: the KT = 10 instance; 3: run-time k."""
    ref = reference(case(batch, d, k, norm))
    with capsys.disabled():
        print()
        check("step API " + ref["c"]["name"], ref, *run_step(ops, ref))


def test_step_api_foreign_entry_among_mixed_positives(ops, capsys):
    """two positives of the batch have an entry that is no corruption of them (another relation; both entities differ): they keep
    `score_independent`, their 89 neighbours the mixed-side path"""
    ref = reference(case(91, 100, 10, "L2", foreign=True))
    with capsys.disabled():
        print()
        check("step API " + ref["c"]["name"], ref, *run_step(ops, ref))


# ---------------------------------------------------------------------------------------------------------------------------------
# the planned epoch call: triple_wave<..., PLAN = true> + apply_step_plan<G, IT, V4>, one worker process under OEA_STEP_PLAN=2
# ---------------------------------------------------------------------------------------------------------------------------------


def worker_main():
    from openea_amd import ops
    ops.lib()
    out = {}
    for ci, c0 in enumerate(json.loads(os.environ["OEA_CASES"])):
        pos, neg, state, c = make_inputs(c0)
        run = sp.DeviceRun(ops, c, pos, neg, np.array([0, len(pos)], np.int64), state)
        got, loss, pad_ok, ws_ok = run.run(0, 1)
        for a in range(4):
            out["%d_%d" % (ci, a)] = got[a]
        out["%d_misc" % ci] = np.array([loss, pad_ok, ws_ok, run.supported], np.float64)
        del run
    np.savez(os.environ["OEA_OUT"], **out)


WORKER = r'''
import os, sys
sys.path[:0] = [os.environ["OEA_ROOT"], os.path.join(os.environ["OEA_ROOT"], "tests")]
import test_mixed_sides_gpu
test_mixed_sides_gpu.worker_main()
'''


def test_planned_epoch_call(tmp_path, capsys):
    """every case above (the foreign-entry one included) through `ops.triple_epoch` with a plan buffer, OEA_STEP_PLAN=2: the plan
    lists no row of these positives, so every row they move goes through the scratch and the flag scan; the relation rows leave
    with the workgroup's sum (at 91 positives the last workgroup's barrier is reached by five waves without a positive)"""
    cases = all_cases()
    refs = [reference(c) for c in cases]
    fout = str(tmp_path / "out.npz")
    env = dict(os.environ, OEA_ROOT=ROOT, OEA_OUT=fout, OEA_CASES=json.dumps(cases))
    for key in ("OEA_STEP_DETERMINISTIC", "OEA_STEP_WAVE", "OEA_STEP_PLAN", "OEA_APPLY_G16", "OEA_APPLY_V4", "OEA_STEP_RUNTIME_KIND",
                "OEA_STEP_REL_ORDER"):
        env.pop(key, None)
    env["OEA_STEP_PLAN"] = "2"
    t0 = time.time()
    p = subprocess.run([sys.executable, "-c", WORKER], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode(errors="replace")[-3000:]
    out = np.load(fout)
    with capsys.disabled():
        print("\nworker: %d cases in %.1f s" % (len(cases), time.time() - t0))
        for ci, ref in enumerate(refs):
            misc = out["%d_misc" % ci]
            assert bool(misc[3]), "%s: the plan was not chosen" % ref["c"]["name"]
            check("planned " + ref["c"]["name"], ref, [out["%d_%d" % (ci, a)] for a in range(4)], float(misc[0]), bool(misc[1]), bool(misc[2]))
