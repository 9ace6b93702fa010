"""The workgroup shape of the planned step: `triple_wave<..., PLAN = true>` in 4-wave workgroups, one positive per wave.

`csrc/triple_step.hip:wave_geometry` launches a planned step at ld <= 128 with 256 threads and one workgroup per 4 positives, up to
`kMaxPlanPartials` = 8,192 workgroups (one loss partial each; `apply_step_plan`'s last block adds them, 32 per lane).
`OEA_STEP_WAVE_BLOCK=512` is the geometry before that rule (8 waves, one workgroup per 8 positives, at most 4,096 partials),
`OEA_STEP_WAVE_BLOCK=256` 4 waves that take two slots each.  Every case runs under all three in one binary, in a process per
setting (the switch is read once), under `OEA_STEP_PLAN=2` (the plan whatever the table size).

Harness and bounds are tests/test_step_plan_gpu.py's: every step on the device and in the C oracle (`oracle.cport.triple_step`),
teacher-forced, workspace / `contrib` / plan not reset in between; `compare()` holds the rows of both tables to the project's 1e-4
(`_tol.assert_rows_close`), the accumulators to rtol 2e-3 / atol 1e-6, the loss to 1e-5 of the oracle's, rows no triple names to
their bits, the pad columns and the scratch to zero.  On top of it the three settings' loss sums agree to 1e-12 relative: they
add the same fp32 per-positive terms in fp64 in three associations of at most 8,192 partials (8,192 * 2^-53 = 9.1e-13).

Shapes (ld 8 and 100; k 10 = the KT = 10 instance, k 3 = the run-time k):
  * batches of 9, 1, 3, 4, 5, 7 and 8 positives: a last workgroup with 1-3 live waves, waves past the end that bring "no row";
  * 4 * 8,192 + 5 positives at ld 8, k 1: the capped grid, a second pass of the grid-stride loop with its barrier, and a last pass
    that one workgroup alone takes (9,000 entities: nearly every row is a hub of the step);
  * relations: "gap" (below), all positives on one relation, every positive on its own relation;
  * the first batch of every small case is built, not drawn: positive 1 is INSIDE BOTH MARGINS (planted rows: head a, relation
    -a/2 + sqrt(3)/2 b, tail their sum, a unit vector -- score 0 <= pos_margin; its negatives all corrupt the tail with the row
    -(tail): score 4 >= neg_margin), positive 2 has a side per negative, and under "gap" the relations are 1 1 1 5 5 1 5 7 7 in
    batch order: in relation order the first workgroup holds relation 1 on waves 0, 2 and 3 with the wave that brings no row
    between them.  The test reads all of that back from float64 scores of the initial tables, not from chance.

Host side, no GPU: `oea_step_workspace_bytes` against the layout restated here.  `loss_partials()` of the non-planned steps has no
C entry point; its callers (`tests/test_kernels_gpu.py`, the "atomic-g16" worker of tests/test_step_plan_gpu.py) hold it.
"""
import os

import numpy as np
import pytest

import test_step_plan_gpu as sp

MAX_PARTIALS, MAX_PLAN_PARTIALS = 4096, 8192      # csrc/step_rows.h: kMaxBlocks, kMaxPlanPartials
PLANT_REL = 1
SETTINGS = {"wg4": {}, "wg8-512": {"OEA_STEP_WAVE_BLOCK": "512"}, "wg4x2-256": {"OEA_STEP_WAVE_BLOCK": "256"}}

_make_batches, _make_tables = sp.make_batches, sp.make_tables


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------


def case(name, rels, plant=True, **kw):
    """rels: per batch, how its relations are drawn -- "rand", "one", "own" or "gap" (module docstring)"""
    c = sp.case(name, **kw)
    c["wg_rels"], c["wg_plant"] = list(rels), bool(plant)
    assert len(c["wg_rels"]) == len(c["sizes"])
    return c


def cases():
    tiny = dict(n_ent=400, n_rel=40, sizes=(9, 1, 3, 4, 5, 7, 8), rels=("gap",) + ("rand",) * 6)
    rels = dict(n_ent=400, n_rel=40, sizes=(9, 11, 9, 6), rels=("gap", "one", "own", "one"), k=10)
    return [case("tiny-d8-k10", d=8, k=10, seed=11, **tiny), case("tiny-d100-k10", d=100, k=10, seed=12, **tiny),
            case("tiny-d8-k3", d=8, k=3, seed=13, **tiny), case("tiny-d100-k3", d=100, k=3, seed=14, **tiny),
            case("rels-d8", d=8, seed=21, **rels), case("rels-d100", d=100, seed=22, **rels),
            case("stride-d8-k1", d=8, k=1, n_ent=9000, n_rel=64, sizes=(4 * MAX_PLAN_PARTIALS + 5,), rels=("rand",), plant=False,
                 seed=31)]


def make_batches(c):
    """-> pos, neg, offsets as sp.make_batches.  Entities uniform over the table without its last three rows (the planted head, tail
    and corrupting row, named by the planted positive alone); a positive's negatives all on one side."""
    if "wg_rels" not in c:
        return _make_batches(c)
    rng = np.random.RandomState(c["seed"])
    n_ent, n_rel, k = c["n_ent"], c["n_rel"], c["k"]
    offsets = np.concatenate([[0], np.cumsum(c["sizes"])]).astype(np.int64)
    n, m = int(offsets[-1]), n_ent - 3
    pos = np.stack([rng.randint(0, m, n), rng.randint(0, n_rel, n), rng.randint(0, m, n)], 1).astype(np.int32)
    for s, mode in enumerate(c["wg_rels"]):
        a, b = int(offsets[s]), int(offsets[s + 1])
        if mode == "one":
            pos[a:b, 1] = PLANT_REL
        elif mode == "own":
            pos[a:b, 1] = rng.permutation(n_rel)[:b - a]
        elif mode == "gap":
            assert b - a == 9
            pos[a:b, 1] = [1, 1, 1, 5, 5, 1, 5, 7, 7]
    side = np.repeat(rng.rand(n) < 0.5, k)                            # True: the head is corrupted
    if c["wg_plant"]:
        assert c["sizes"][0] >= 3 and k >= 2
        side[2 * k: 3 * k] = np.arange(k) % 2 == 0                    # positive 2: a side per negative
    ne = rng.randint(0, m, n * k)
    neg = np.repeat(pos, k, 0)
    neg[side, 0] = ne[side]
    neg[~side, 2] = ne[~side]
    if c["wg_plant"]:
        pos[1] = (m, PLANT_REL, m + 1)                                # inside both margins on make_tables' rows
        neg[k: 2 * k] = (m, PLANT_REL, m + 2)
    return pos, neg.astype(np.int32), offsets


def make_tables(c):
    state = _make_tables(c)
    if c.get("wg_plant"):
        ent, rel, d, m = state[0], state[2], c["d"], c["n_ent"] - 3
        a, b = np.zeros(d), np.zeros(d)
        a[0], b[1] = 1.0, 1.0
        ent[m], rel[PLANT_REL] = a, -0.5 * a + np.sqrt(0.75) * b
        ent[m + 1] = 0.5 * a + np.sqrt(0.75) * b
        ent[m + 2] = -ent[m + 1]
    return state


WORKER = r'''
import os, sys
sys.path[:0] = [os.environ["OEA_ROOT"], os.path.join(os.environ["OEA_ROOT"], "tests")]
import test_wave_workgroup_gpu as t
t.sp.make_batches, t.sp.make_tables = t.make_batches, t.make_tables
t.sp.worker_main()
'''


@pytest.fixture(autouse=True)
def _own_inputs(monkeypatch):
    """the helpers of test_step_plan_gpu draw batches and tables through its module-level names; the switches under test come from
    SETTINGS alone"""
    monkeypatch.setattr(sp, "make_batches", make_batches)
    monkeypatch.setattr(sp, "make_tables", make_tables)
    monkeypatch.setattr(sp, "WORKER", WORKER)
    for key in ("OEA_STEP_WAVE_BLOCK", "OEA_STEP_REL_ORDER", "OEA_STEP_WAVE_DBG"):
        monkeypatch.delenv(key, raising=False)


# ---------------------------------------------------------------------------------------------------------------------------------
# what the first batch was built for, read back from float64 scores
# ---------------------------------------------------------------------------------------------------------------------------------


def first_batch_facts(c, state, pos, neg):
    """-> active[i]: positive i of the batch brings a relation row (its own term or one of its negatives is active)"""
    k, l1 = c["k"], c["norm"] == "L1"
    pm, nm = float(np.float32(c["pos_margin"])), float(np.float32(c["neg_margin"]))
    sp_, sn = sp._scores64(state[0], state[2], pos, l1), sp._scores64(state[0], state[2], neg, l1).reshape(len(pos), k)
    return (sp_ > pm) | (sn < nm).any(1), sp_, sn


def check_built_batch(c, traj, pos, neg, offsets):
    hi = int(offsets[1])
    p, g = pos[:hi], neg[:hi * c["k"]]
    active, s_pos, s_neg = first_batch_facts(c, traj[0][1], p, g)
    assert not active[1] and s_pos[1] < 1e-9 and s_neg[1].min() > 3.99, "the planted positive is not inside both margins"
    assert active[np.arange(hi) != 1].all(), "a positive next to the planted one brings no row"
    ng = g.reshape(hi, c["k"], 3)
    keeps_head = ng[2, :, 0] == p[2, 0]
    assert keeps_head.any() and not keeps_head.all(), "positive 2 is not mixed-side"
    if c["wg_rels"][0] == "gap":
        order = np.argsort(p[:, 1], kind="stable")
        assert list(order[:4]) == [0, 1, 2, 5] and list(p[order[:4], 1]) == [PLANT_REL] * 4    # workgroup 0: rows on waves 0, 2, 3
        assert len(np.unique(p[order[4:8], 1])) == 2                                          # an 8-wave workgroup holds three


# ---------------------------------------------------------------------------------------------------------------------------------
# the test
# ---------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("ci", range(len(cases())), ids=[c["name"] for c in cases()])
def test_planned_step_in_every_workgroup_shape(ci, tmp_path, capsys):
    all_cases = cases()
    c = all_cases[ci]
    pos, neg, offsets = make_batches(c)
    with capsys.disabled():
        print()
        traj = sp.oracle_steps(c, pos, neg, offsets)
        if c["wg_plant"]:
            check_built_batch(c, traj, pos, neg, offsets)
        if c["name"].startswith("stride"):
            n = c["sizes"][0]
            assert n > 4 * MAX_PLAN_PARTIALS and n % 4 != 0 and -(-n // 8) > MAX_PARTIALS    # every setting's grid is capped
        losses = {}
        for tag, extra in SETTINGS.items():
            out, factory = sp.run_worker(tmp_path, "wave-" + tag, dict(OEA_STEP_PLAN="2", **extra), all_cases)
            assert bool(out["%d_supported" % ci]), "%s: no plan under OEA_STEP_PLAN=2" % c["name"]
            run_call = factory(ci)
            losses[tag] = []
            for s, before, after, loss_ref, facts in traj:
                got, loss, pad_ok, ws_ok = run_call(s, s, s + 1, None)
                sp.compare("%s %s step %d (%d positives)" % (tag, c["name"], s, c["sizes"][s]), c, before, got, after, loss, loss_ref,
                           pad_ok, ws_ok, facts["named_ent"], facts["named_rel"], facts["skip_ent"], facts["skip_rel"])
                losses[tag].append(loss)
        for s in range(len(traj)):
            three = [losses[tag][s] for tag in SETTINGS]
            spread = max(three) - min(three)
            print("%s step %d: loss %s, spread %.3g relative" % (c["name"], s, three, spread / max(abs(max(three)), 1e-300)))
            assert spread <= 1e-12 * max(abs(x) for x in three), "%s step %d: loss sums %r" % (c["name"], s, three)


def test_workspace_grows_by_the_added_partials_only():
    """the step workspace = the layout of csrc/step_rows.h:ws_layout restated (256-byte aligned pieces: entity / relation / normal
    scratch, three flag arrays, 15 extra copies of the relation and of the normal scratch) + the loss partials: 4,096 doubles before
    the planned step's were added, at most 8,192 now"""
    from openea_amd import _lib
    lib = _lib.load(require_device=False)
    el = lib.oea_step_scratch_elem_bytes()

    def al(x):
        return (x + 255) // 256 * 256
    for n_ent, n_rel, ld in ((1, 1, 4), (400, 40, 8), (6000, 200, 76), (200000, 700, 100), (1200000, 200, 8)):
        rest = al(el * n_ent * ld) + 2 * al(el * n_rel * ld) + al(el * n_ent) + 2 * al(el * n_rel) + 2 * al(el * n_rel * ld * 15)
        got = lib.oea_step_workspace_bytes(n_ent, n_rel, ld)
        assert rest + 8 * MAX_PARTIALS < got <= rest + 8 * MAX_PLAN_PARTIALS, (n_ent, n_rel, ld, got, rest)
