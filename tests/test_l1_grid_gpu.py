"""GPU parity tests of the 16-bit grid Manhattan prefilter, piece by piece: the quantiser, the integer strip, the two exact pair
kernels, the error bound of a grid distance on a table built to spend it, the two rank kernels on strips chosen by hand (the
honest one, one that misleads as far as the certificate allows, one ordered so that the running-minimum list overflows), the
certified lists' fallback count, and the ranking select on rows with NaN and +-inf.

Every piece of this path sits in front of an exact all-pairs fallback, so the end-to-end tests (tests/test_kernels_gpu.py,
tests/test_gnn_gpu.py) cannot tell a broken piece from a working one.  Here each piece is called by name and held to a numpy
restatement on the host: int64 for grid sums, fp64 for distances.  Every buffer a kernel stores to is pre-filled with NaN or a
sentinel, the padding columns of every source table hold NaN, every bound is written next to its assert, and each test prints
max(measured / bound)."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32 = np.float32
U32 = 2.0 ** -24                      # fp32 unit roundoff
U64 = 2.0 ** -53                      # fp64 unit roundoff
K_AMB, K_TOP = 2048, 4096             # l1_grid.hip kGridAmb / kGridTop: the capacities of a row's two candidate lists
SENT = 7.0                            # strip sentinel: a strip holds -G <= -0.0, never a positive value


@pytest.fixture(scope="module")
def ops():
    from openea_amd import ops as _ops
    _ops.lib()   # raises loudly if the HIP library / GPU is missing
    return _ops


# ---------------------------------------------------------------------------------------------
# host restatements (pure numpy: they run without a GPU)
# ---------------------------------------------------------------------------------------------
def _pad(n, m):
    return (n + m - 1) // m * m


def quantize_ref(x, lo, inv_step):
    """quantize_rows_u16_kernel, bit for bit: two fp32 roundings (the subtraction, the product; nothing to fuse), rintf = round
    half to even = np.rint, clamp"""
    t = (np.asarray(x, F32) - F32(lo)) * F32(inv_step)
    return np.clip(np.rint(t), F32(0), F32(65535)).astype(np.uint16)


def grid_sums(qa, qb):
    """sum_k |qa[i, k] - qb[j, k]| in int64"""
    a, b = qa.astype(np.int64), qb.astype(np.int64)
    out = np.zeros((a.shape[0], b.shape[0]), np.int64)
    for k in range(a.shape[1]):
        out += np.abs(a[:, k, None] - b[None, :, k])
    return out


def seq_l1(a, b):
    """fp64 L1 distances [n1, n2] of fp32 rows with the SEQUENTIAL chain, k ascending (exact_l1_sim / pair_l1_sim_seq_kernel /
    scipy's cdist)"""
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
    acc = np.zeros((a64.shape[0], b64.shape[0]))
    for k in range(a64.shape[1]):
        acc += np.abs(a64[:, k, None] - b64[None, :, k])
    return acc


def seq_l1_pairs(a, b):
    """the same chain for row pairs a[p], b[p]"""
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
    acc = np.zeros(a64.shape[0])
    for k in range(a64.shape[1]):
        acc += np.abs(a64[:, k] - b64[:, k])
    return acc


def butterfly_l1_pairs(a, b):
    """pair_l1_f64_kernel's order: lane l of 16 adds columns l, l + 16, ... in turn, then the xor butterfly 8, 4, 2, 1"""
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n, d = a64.shape
    part = np.zeros((n, 16))
    for k in range(d):
        part[:, k % 16] += np.abs(a64[:, k] - b64[:, k])
    lanes = np.arange(16)
    for off in (8, 4, 2, 1):
        part = part + part[:, lanes ^ off]
    return part[:, 0]


def sim32(d64):
    return (1.0 - d64).astype(F32)


def ref_rank_argmax(v, gold):
    """rank_valu_kernel's answers from a full row of values: rank = candidates that beat the gold (larger value, or the same value
    in an earlier column), nearest = the largest value, ties to the earlier column"""
    n, nc = v.shape
    vg = v[np.arange(n), gold][:, None]
    j = np.arange(nc)[None, :]
    rank = ((v > vg) | ((v == vg) & (j < gold[:, None]))).sum(1).astype(np.int32)
    return rank, np.argmax(v, axis=1).astype(np.int32)


def plain_tol(sg, step, err):
    """rank_l1_grid_rows_kernel's slack around the gold distance, in fp32 as the kernel computes it -> (dg, tol)"""
    step, err = F32(step), F32(err)
    tol = (err + F32(4.0e-7) * np.maximum(np.abs(sg), F32(1.0))) + F32(4.0) * step
    return (1.0 - sg.astype(np.float64)).astype(F32), tol


def plain_counts(G, gold, sg, step, err):
    """what the plain kernel will find in a strip G [n, nc] (grid units): per row the number of ambiguous candidates and the
    number within the band of the row's smallest grid distance"""
    G = G.astype(F32)
    dg, tol = plain_tol(sg, step, err)
    g_lo, g_hi, band = (dg - tol) / F32(step), (dg + tol) / F32(step), F32(2.0) * tol / F32(step)
    amb = (G >= g_lo[:, None]) & (G <= g_hi[:, None])
    amb[np.arange(G.shape[0]), gold] = False
    top = G <= (G.min(1) + band)[:, None]
    return amb.sum(1), top.sum(1)


def csls_bounds(G, r, c, step, err):
    """rank_l1_grid_rows_csls_kernel's interval of every candidate -> (lower, upper) fp32 [n, nc]"""
    step32, err32 = F32(step), F32(err)
    sa = (1.0 - G.astype(np.float64) * float(step32)).astype(F32)                 # fmaf(-G, step, 1)
    va = (F32(2.0) * sa - r[:, None]) - c[None, :]
    tol = (F32(2.0) * err32 + F32(8.0) * step32) + F32(6.0e-7) * (((F32(2.0) * np.abs(sa) + np.abs(r)[:, None]) + np.abs(c)[None, :]) + F32(1.0))
    return va - tol, va + tol


def csls_counts(G, gold, vg, r, c, step, err):
    lower, upper = csls_bounds(G, r, c, step, err)
    amb = ~(lower > vg[:, None]) & (upper >= vg[:, None])
    amb[np.arange(G.shape[0]), gold] = False
    top = upper >= lower.max(1)[:, None]
    return amb.sum(1), top.sum(1)


def first_pass_records(nc, keep, fold):
    """the first pass of either rank kernel over ONE strip row: thread t owns columns 4 t .. 4 t + 3 (+ 1,024, ...) in ascending
    order, records a column when keep(j, running) holds (always while it has seen nothing: the running extreme starts at
    infinity), then folds the column into its running extreme -> the number of records"""
    n = 0
    for t in range(256):
        run = None
        for j4 in range(4 * t, nc, 1024):
            for j in range(j4, min(j4 + 4, nc)):
                n += 1 if run is None or keep(j, run) else 0
                run = fold(j, run)
    return n


def misleading_strip(d64, better, gold, step, err):
    """G_j = rint(d_j / step + s_j (err / step - 1)): s_j = +1 (looks farther) for the candidates that beat the gold, -1 (looks
    nearer) for the others, the gold itself honest.  Every entry stays within err of the truth and points the wrong way."""
    step, err = float(F32(step)), float(F32(err))
    s = np.where(better, 1.0, -1.0)
    s[np.arange(d64.shape[0]), gold] = 0.0
    G = np.maximum(np.rint(d64 / step + s * (err / step - 1.0)), 0.0)
    assert np.all(np.abs(G * step - d64) <= err - 0.4 * step)                     # rint moves it by at most half a step
    assert G.max() < 2 ** 24                                                       # exactly representable in the fp32 strip
    return G.astype(np.int64)


def restate_topk_means_uncertified(G, sims, k, margin, step, err):
    """ops.l1_grid_topk_means' certificate from the integer strip G [n, nc] and the exact fp32 similarities sims [n, nc] of every
    pair: the list = the k + margin smallest grid distances (ties: smaller column, oea_topk_rows' rule), a row is redone when the
    bound of a non-member, 1 - (worst step - (err + 4 step)), exceeds the list's k-th largest exact similarity -> bool [n]"""
    n, nc = G.shape
    c = min(k + margin, nc)
    if c >= nc:
        return np.zeros(n, bool)
    cand = np.sort(np.argsort(G, axis=1, kind="stable")[:, :c], axis=1)
    worst = np.take_along_axis(G, cand, 1).max(1).astype(np.float64)
    kth = -np.sort(-np.take_along_axis(sims, cand, 1), axis=1)[:, k - 1]
    bound = 1.0 - (worst * step - (err + 4.0 * step))
    return ~(bound <= kth.astype(np.float64))


def restate_get_neg_uncertified(G, table, seeds, dim, k, margin, step):
    """approaches/rdgcn.py:get_neg's certificate: the list's worst grid distance minus (1.02 dim + 4) steps must lie above the
    k-th smallest exact distance of the list (pair_l1_f64_kernel's butterfly order) -> (bool [t], smallest |bound - kth|)"""
    c = k + margin
    cand = np.sort(np.argsort(G, axis=1, kind="stable")[:, :c], axis=1)
    worst = np.take_along_axis(G, cand, 1).max(1).astype(np.float64)
    bound = worst * step - (dim * 1.02 + 4.0) * step
    q = np.repeat(table[seeds, :dim], c, axis=0)
    d = butterfly_l1_pairs(q, table[cand.reshape(-1), :dim]).reshape(len(seeds), c)
    kth = np.sort(d, axis=1)[:, k - 1]
    return ~(bound > kth), np.abs(bound - kth).min()


# ---------------------------------------------------------------------------------------------
# device helpers
# ---------------------------------------------------------------------------------------------
def _table(ops, a, ld=None):
    """ops.to_table with the padding columns overwritten by NaN: nothing may read them"""
    t = ops.to_table(a, ld)
    if t.shape[1] > a.shape[1]:
        t[:, a.shape[1]:] = float("nan")
    return t


def _u16(ops, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint16).view(np.int16)).to(ops.device())


def _host_u16(t):
    return t.cpu().numpy().view(np.uint16)


def _bits32(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---------------------------------------------------------------------------------------------
# 1. quantize_rows_u16
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 257])
@pytest.mark.parametrize("dim", [1, 7, 8, 9, 75, 300, 1200])
def test_quantize_rows_u16_is_the_fp32_map_bit_for_bit(ops, dim, rows):
    """oea_quantize_rows_u16 == clip(rint((x - float32(lo)) * float32(inv_step)), 0, 65535) in numpy float32 on all ldq columns
    (padding 0), on a binary grid (lo = -2, step = 2^-13: the map is exact, so lo / hi land on 0 / 65535 and planted half-steps on
    the even neighbour) and on a grid as L1Grid derives it from a table's range; against the fp64 ideal every element inside the
    range lies within (0.5 + 3 * 2^-24 * 65535) steps of its grid point (the three fp32 roundings: inv_step, x - lo, the product)."""
    rng = np.random.RandomState(100 * dim + rows)
    ldq = _pad(dim, 8)
    worst = 0.0
    for grid in ("binary", "range"):
        if grid == "binary":
            lo, step = -2.0, 2.0 ** -13
            hi = lo + 65535 * step
        else:
            lo, hi = float(F32(-0.7313)), float(F32(1.2709))
            step = (hi - lo) / 65535.0
        inv_step = float(F32(1.0 / step))
        x = (lo + rng.rand(rows, dim) * (hi - lo)).astype(F32)
        flat = x.reshape(-1)
        plant = {}
        flat[0] = lo
        plant[0] = 0
        if flat.size > 1:
            flat[-1] = hi
            plant[flat.size - 1] = 65535
        if flat.size > 8:
            flat[1], flat[2] = F32(lo - 3.0 * step), F32(hi + 3.0 * step)             # outside the range: clamped
            plant[1], plant[2] = 0, 65535
        if grid == "binary" and flat.size > 8:
            for at, m in ((3, 0), (4, 1), (5, 2), (6, 40001), (7, 65534)):            # m + 0.5 -> the even one of m, m + 1
                flat[at] = F32(lo + (m + 0.5) * step)
                assert float(flat[at]) == lo + (m + 0.5) * step                       # representable: the map is exact
                plant[at] = m + (m & 1)
        src = _table(ops, x, ld=_pad(dim, 4) + 4)
        dst = torch.full((rows, ldq), -1, dtype=torch.int16, device=ops.device())      # 0xFFFF: neither a pad value nor likely
        ops.check(ops.lib().oea_quantize_rows_u16(ops._p(src), rows, src.shape[1], dim, lo, inv_step, ops._p(dst), ldq, ops._stream()))
        got = _host_u16(dst)
        ref = quantize_ref(x, lo, inv_step)
        assert np.array_equal(got[:, :dim], ref), (grid, np.argwhere(got[:, :dim] != ref)[:4])
        assert not got[:, dim:].any()                                                  # pad columns: the same grid point in every row
        for at, q in plant.items():
            assert got[:, :dim].reshape(-1)[at] == q, (grid, at, q)
        inside = (x >= F32(lo)) & (x <= F32(hi))
        dev = np.abs(x.astype(np.float64) - (lo + got[:, :dim].astype(np.float64) * step))[inside]
        bound = (0.5 + 3 * U32 * 65535) * step
        assert dev.max() <= bound, (grid, dev.max() / step)
        worst = max(worst, dev.max() / bound)
    print("quantize_rows_u16 dim %d rows %d: max(|x - (lo + q step)| / bound) = %.4f" % (dim, rows, worst))


# ---------------------------------------------------------------------------------------------
# 2. l1_u16_strip
# ---------------------------------------------------------------------------------------------
def _strip_case(ops, qa, qb, ld_out, extra_rows=3):
    nq, nc = qa.shape[0], qb.shape[0]
    out = torch.full((nq + extra_rows, ld_out), SENT, dtype=torch.float32, device=ops.device())
    da, db = _u16(ops, qa), _u16(ops, qb)
    ops.check(ops.lib().oea_l1_u16_strip(ops._p(da), nq, ops._p(db), nc, qa.shape[1], ops._p(out), ld_out, ops._stream()))
    got = out.cpu().numpy()
    ref = -(grid_sums(qa, qb).astype(F32))                       # int64 -> fp32 rounds to nearest even, like the u32 conversion
    assert np.array_equal(_bits32(got[:nq, :nc]), _bits32(ref)), np.argwhere(_bits32(got[:nq, :nc]) != _bits32(ref))[:4]
    assert np.all(_bits32(got[:nq, nc:]) == _bits32(F32(SENT))) and np.all(_bits32(got[nq:]) == _bits32(F32(SENT)))


@pytest.mark.parametrize("ldq", [8, 64, 72, 304, 1200])
@pytest.mark.parametrize("nq,nc", [(1, 1), (127, 129), (128, 128), (129, 257), (257, 127)])
def test_l1_u16_strip_equals_integer_sums(ops, nq, nc, ldq):
    """oea_l1_u16_strip == -float32(sum_k |qa - qb|) bit for bit ([nq, nc] around the 128 x 128 tile; ldq: less than a staged
    chunk of 32 dwords, one chunk, a chunk and a remainder of 4, several), with the row pitch padded to 32 (16-byte stores) and
    equal to nc (the scalar stores when nc % 4 != 0); everything outside [nq, nc] keeps its sentinel."""
    rng = np.random.RandomState(nq * 1000 + nc + ldq)
    qa = rng.randint(0, 65536, (nq, ldq)).astype(np.uint16)
    qb = rng.randint(0, 65536, (nc, ldq)).astype(np.uint16)
    for ld_out in (_pad(nc, 32), nc):
        _strip_case(ops, qa, qb, ld_out)
    print("l1_u16_strip %d x %d x %d: max(measured / bound) = 0 (bit-equal)" % (nq, nc, ldq))


def test_l1_u16_strip_rounds_sums_past_2_to_24_like_the_host(ops):
    """all 0 against all 65535 at 1,200 columns (78,642,000 = 2^4 * 4,915,125: still an fp32 value) and, beside it, rows whose
    last entry is a little smaller: sums between 2^26 and 2^27, where fp32 values are 8 apart -- 78,641,999 (rounds up),
    78,641,996 (exactly half way: to the even neighbour) and 78,641,995 (rounds down); the strip holds what the host's
    int64 -> fp32 conversion gives"""
    qa, qb = np.zeros((5, 1200), np.uint16), np.full((131, 1200), 65535, np.uint16)
    qb[3, -1], qb[4, -1], qb[5, -1] = 65534, 65531, 65530
    qb[7, :600] = 0                                               # and a sum below 2^24 next to them
    sums = grid_sums(qa, qb)[0]
    assert sums[0] == 78642000 and [int(F32(x)) - int(x) for x in sums[3:6]] == [1, 4, -3]
    assert int(F32(78641992)) == 78641992                         # 78,641,996 is a tie between two fp32 values ...
    assert (F32(78642000).view(np.uint32) & 1) == 0               # ... and went to the one with the even significand
    for ld_out in (_pad(131, 32), 131):
        _strip_case(ops, qa, qb, ld_out)
    print("l1_u16_strip saturated: max(measured / bound) = 0 (bit-equal)")


# ---------------------------------------------------------------------------------------------
# 3. pair_l1_sim / pair_l1_f64
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 42])
@pytest.mark.parametrize("dim", [1, 15, 16, 17, 75, 300])
def test_pair_l1_kernels_against_fp64_chains(ops, dim, c):
    """oea_pair_l1_sim == float32(1 - acc) of the host chain acc += |a_k - b_k| (k ascending, fp64) bit for bit; oea_pair_l1_f64
    within (dim - 1) * 2^-53 * sum|terms| of math.fsum (its butterfly order gets a bound, not bits), equal pairs equal bits.
    13 query rows (13 and 546 pairs: no multiple of 16 or 256), candidate lists with repeats, ids 0 and n - 1, and the query row
    itself: distance 0.0, similarity exactly 1.0."""
    rng = np.random.RandomState(dim * 10 + c)
    n, nq = 97, 13
    # entries over 26 binades: fp64 sums of such terms round at every step, so the order of the chain shows in the bits (sums of
    # fp32 values of one magnitude are exact in fp64 in any order and would let a wrong order pass)
    tab = (rng.standard_normal((n, dim)) * 0.3 * 2.0 ** rng.randint(-20, 7, (n, dim))).astype(F32)
    qid = rng.choice(n, nq, replace=False)
    cand = rng.randint(0, n, (nq, c)).astype(np.int32)
    if c == 1:
        cand[:5, 0] = qid[:5]
        cand[5, 0], cand[6, 0] = 0, n - 1
    else:
        cand[:, 0] = qid                                          # the query row itself
        cand[:, 1], cand[:, 2] = 0, n - 1
        cand[:, 5] = cand[:, 4]                                   # a repeat in every list
        cand[:, 7] = qid
    t = _table(ops, tab)
    q = _table(ops, tab[qid], ld=_pad(dim, 4) + 4)
    dc = ops.to_ids(cand)
    sim = torch.full((nq, c), float("nan"), dtype=torch.float32, device=ops.device())
    d64 = torch.full((nq, c), float("nan"), dtype=torch.float64, device=ops.device())
    ops.check(ops.lib().oea_pair_l1_sim(ops._p(q), nq, q.shape[1], ops._p(t), n, t.shape[1], dim, ops._p(dc), c, ops._p(sim), ops._stream()))
    ops.check(ops.lib().oea_pair_l1_f64(ops._p(q), nq, q.shape[1], ops._p(t), n, t.shape[1], dim, ops._p(dc), c, ops._p(d64), ops._stream()))
    sim, d64 = sim.cpu().numpy(), d64.cpu().numpy()
    a, b = np.repeat(tab[qid], c, axis=0), tab[cand.reshape(-1)]
    ref_sim = sim32(seq_l1_pairs(a, b)).reshape(nq, c)
    if dim >= 15 and c > 1:                                       # the order matters on this table: the reversed chain differs
        assert np.any(seq_l1_pairs(a[:, ::-1], b[:, ::-1]) != seq_l1_pairs(a, b))
    assert np.array_equal(_bits32(sim), _bits32(ref_sim))
    terms = np.abs(a.astype(np.float64) - b.astype(np.float64))
    exact = np.array([math.fsum(row) for row in terms]).reshape(nq, c)
    bound = (dim - 1) * U64 * terms.sum(1).reshape(nq, c)          # dim - 1 additions, each within 2^-53 of its partial sum
    err = np.abs(d64 - exact)
    assert np.all(err <= bound), (err - bound).max()
    own = cand == qid[:, None]
    assert own.any() and np.all(d64[own] == 0.0) and np.all(sim[own] == F32(1.0))
    if c > 1:
        assert np.array_equal(d64[:, 5], d64[:, 4]) and np.array_equal(sim[:, 5], sim[:, 4])
    ratio = (err[bound > 0] / bound[bound > 0]).max() if (bound > 0).any() else 0.0
    print("pair_l1 dim %d c %d: similarities bit-equal; fp64 distances max(err / bound) = %.4f" % (dim, c, ratio))


# ---------------------------------------------------------------------------------------------
# 4. the error bound of a grid distance on a table built to spend it
# ---------------------------------------------------------------------------------------------
def adversarial_tables(d, n=48, seed=0):
    """48 query and 48 candidate rows that push every column's two rounding errors the same way: query entries at
    lo + (q + 0.49) step (rounded DOWN by 0.49), candidate entries at lo + (q' - 0.49) step with q' < q (rounded UP by 0.49), so
    every column's grid difference q - q' falls 0.98 steps short of the true one.  All grid points in the upper half of the grid,
    where the fp32 map's absolute rounding is largest; one entry each pinned to the range ends.  (0.49 is as near to a half as
    fp32 tables allow here: an entry's own spacing is ~0.004 steps and the map adds up to 0.01.)"""
    rng = np.random.RandomState(seed + d)
    lo, hi = float(F32(-0.7313)), float(F32(1.2709))
    step = (hi - lo) / 65535.0
    qq = rng.randint(49152, 65535, (n, d))
    qc = rng.randint(32768, 49152, (n, d))
    e1 = (lo + (qq + 0.49) * step).astype(F32)
    e2 = (lo + (qc - 0.49) * step).astype(F32)
    e1[0, 0], e2[0, 0] = hi, lo
    return e1, e2, lo, hi, step


@pytest.mark.parametrize("d", [8, 75, 300, 1200])
def test_grid_error_bound_holds_on_an_adversarial_table(ops, d):
    """max |G step - d_fp64| over all pairs, G from the device strip of ops.L1Grid, on adversarial_tables(d): <= L1Grid.err, and
    <= get_neg's (1.02 d + 4) step; the table really presses on the bound (>= 0.95 d steps) while an ideal fp64 quantiser alone
    stays within d steps."""
    from scipy.spatial.distance import cdist
    e1, e2, lo, hi, step = adversarial_tables(d)
    d64 = cdist(e1.astype(np.float64), e2.astype(np.float64), "cityblock")
    ideal = lambda e: np.clip(np.rint((e.astype(np.float64) - lo) / step), 0, 65535).astype(np.uint16)
    dev_ideal = np.abs(grid_sums(ideal(e1), ideal(e2)) * step - d64).max() / step
    assert dev_ideal <= d, dev_ideal                               # half a step per operand and column
    grid = ops.L1Grid(_table(ops, e1), _table(ops, e2), d)
    assert grid.step == step
    n = e1.shape[0]
    G = -grid.strip(0, n).cpu().numpy()[:, :n].astype(np.float64)
    # (the strip is fp32: from d = 1,200 on these sums pass 2^24 and the measure includes their rounding, as the consumers see it)
    assert np.array_equal(G, grid_sums(quantize_ref(e1, lo, 1.0 / step), quantize_ref(e2, lo, 1.0 / step)).astype(F32))
    dev = np.abs(G * step - d64).max()
    steps = dev / step
    assert steps >= 0.95 * d, steps                                # the construction spends the budget
    assert dev <= grid.err, (steps, grid.err / step)               # (1.02 d + 1) step
    assert dev <= (d * 1.02 + 4.0) * step                          # get_neg's form of the bound
    print("grid bound d %d: deviation %.1f steps (fp64-ideal quantiser %.1f) of L1Grid.err %.1f: max(measured / bound) = %.4f"
          % (d, steps, dev_ideal, grid.err / step, dev / grid.err))


# ---------------------------------------------------------------------------------------------
# 5. the two rank kernels alone, on strips chosen by hand
# ---------------------------------------------------------------------------------------------
GRID_LO, GRID_STEP = -4.0, 2.0 ** -12            # the tables of this section span [lo, lo + 65535 step] exactly


def _rank_tables(d, nc, seed):
    """n1 query and nc candidate rows on a narrow cloud (spread: a few times the grid's error bound wide in distance, so that
    every row has candidates the grid cannot decide) inside a range pinned by two entries of query row 0; gold of row i = column
    off + i; exact duplicates of gold columns in front of the golds and behind them."""
    rng = np.random.RandomState(seed)
    n1, off = {1: (1, 0), 255: (40, 100), 1031: (300, 700)}[nc]
    spread = 40 if d < 8 else 100
    point = lambda n: (GRID_LO + (40000 + np.round(rng.rand(n, d) * spread * 256) / 256) * GRID_STEP).astype(F32)
    e1, e2 = point(n1), point(nc)
    e1[0, 0], e1[0, 1] = GRID_LO, GRID_LO + 65535 * GRID_STEP
    dups = {1: (), 255: ((10, 100, 10), (200, 120, 10)), 1031: ((0, 700, 50), (1000, 800, 31))}[nc]      # (to, from, rows)
    for to, frm, n in dups:
        e2[to: to + n] = e2[frm: frm + n]
    return e1, e2, off, dups


def _run_rank(ops, strip, nc, fill, blocks, t1, t2, d, off, step, err, csls=None):
    """one launch per block of query rows (row0, rows) on the strip's rows, its columns >= nc filled with `fill` -> rank, argmax
    (sentinel -7 where no block wrote), n_exact_rows"""
    n1, ld = strip.shape
    dev = ops.device()
    s = strip.clone()
    s[:, nc:] = fill
    rank = torch.full((t1.shape[0],), -7, dtype=torch.int32, device=dev)
    arg = torch.full((t1.shape[0],), -7, dtype=torch.int32, device=dev)
    n_exact = torch.zeros(1, dtype=torch.int32, device=dev)
    for row0, rows in blocks:
        sub = s[row0: row0 + rows].contiguous()
        if csls is None:
            ops.check(ops.lib().oea_rank_l1_grid_rows(ops._p(sub), rows, row0, nc, ld, ops._p(t1), t1.shape[1], ops._p(t2), t2.shape[1],
                                                      d, off, float(step), float(err), ops._p(rank), ops._p(arg), ops._p(n_exact),
                                                      ops._stream()))
        else:
            ops.check(ops.lib().oea_rank_l1_grid_rows_csls(ops._p(sub), rows, row0, nc, ld, ops._p(t1), t1.shape[1], ops._p(t2),
                                                           t2.shape[1], d, off, float(step), float(err), ops._p(csls[0]),
                                                           ops._p(csls[1]), ops._p(rank), ops._p(arg), ops._p(n_exact), ops._stream()))
    return rank.cpu().numpy(), arg.cpu().numpy(), int(n_exact.item())


def _dev_strip(ops, G, ld):
    s = torch.full((G.shape[0], ld), float("nan"), dtype=torch.float32, device=ops.device())
    s[:, :G.shape[1]] = torch.from_numpy(-(G.astype(F32))).to(ops.device())
    return s


FILLS = (float("nan"), -0.0, -1e30)              # what the strip's columns >= nc hold: NaN, a grid distance of 0, of 1e30


@pytest.mark.parametrize("nc", [1, 255, 1031])
@pytest.mark.parametrize("d", [3, 75, 300])
def test_rank_kernels_decide_exactly_on_honest_and_misleading_strips(ops, d, nc):
    """oea_rank_l1_grid_rows and _csls, called alone: ranks and nearest candidates == the all-pairs fp64 answers (sequential
    chain, the kernels' tie rule) with n_exact_rows == 0, on the device strip and on a strip that misleads as far as the
    certificate allows (every entry within err of the truth, pointing the wrong way); d odd and even (the padding of the
    query row in LDS), nc below the thread count and with nc % 4 == 3, the strip's columns >= nc filled with NaN / -0.0 / -1e30,
    one row, row0 > 0 with a gold offset, duplicates of gold columns on both sides; CSLS means ~ U(0, 0.3) and negative ones."""
    e1, e2, off, dups = _rank_tables(d, nc, seed=1000 * d + nc)
    n1 = e1.shape[0]
    rng = np.random.RandomState(d + nc)
    t1, t2 = _table(ops, e1, ld=_pad(d, 4) + 4), _table(ops, e2)
    grid = ops.L1Grid(t1, t2, d)
    assert grid.step == GRID_STEP
    step, err, ld = grid.step, grid.err, grid.ld
    honest = grid.strip(0, n1)
    G = grid_sums(quantize_ref(e1, GRID_LO, 1.0 / GRID_STEP), quantize_ref(e2, GRID_LO, 1.0 / GRID_STEP))
    assert np.array_equal(-honest.cpu().numpy()[:, :nc], G.astype(F32))
    d64 = seq_l1(e1, e2)
    s = sim32(d64)
    gold = (off + np.arange(n1)).astype(np.int64)
    blocks_all = [[(0, n1)]] if n1 == 1 else [[(0, n1)], [(7, 1)], [(n1 // 2, n1 - n1 // 2)]]
    jj = np.arange(nc)[None, :]
    worst = 0.0
    for name, means in (("plain", None), ("csls", (0.0, 0.3)), ("csls-", (-0.3, 0.0))):
        if means is None:
            v, csls = s, None
        else:
            r = rng.uniform(means[0], means[1], n1).astype(F32)
            c = rng.uniform(means[0], means[1], nc).astype(F32)
            for to, frm, n in dups:
                c[to: to + n] = c[frm: frm + n]                       # a duplicate ties with its gold under CSLS too
            v = (F32(2.0) * s - r[:, None]) - c[None, :]
            csls = (ops.to_vec(r), ops.to_vec(c))
        ref_rank, ref_arg = ref_rank_argmax(v, gold)
        vg = v[np.arange(n1), gold]
        assert nc == 1 or ((v == vg[:, None]).sum() - n1) >= 20        # the tie rule is exercised
        better = (v > vg[:, None]) | ((v == vg[:, None]) & (jj < gold[:, None]))
        Gm = misleading_strip(d64, better, gold, step, err)
        for kind, Gs, strip in (("honest", G, honest), ("misleading", Gm, _dev_strip(ops, Gm, ld))):
            namb, ntop = plain_counts(Gs, gold, vg, step, err) if means is None else csls_counts(Gs, gold, vg, r, c, step, err)
            # neither list may overflow (the kernel then answers from all pairs, which proves nothing about the lists) ...
            assert namb.max() < K_AMB and ntop.max() < K_TOP
            if kind == "misleading" and nc > 1:
                assert namb.min() > 0, (name, namb.min())           # ... and the misleading strip must leave a doubt in every row
            worst = max(worst, namb.max() / K_AMB, ntop.max() / K_TOP)
            for fill in FILLS:
                for blocks in blocks_all:
                    rank, arg, n_exact = _run_rank(ops, strip, nc, fill, blocks, t1, t2, d, off, step, err, csls)
                    rows = np.concatenate([np.arange(r0, r0 + n) for r0, n in blocks])
                    what = (name, kind, fill, blocks)
                    assert n_exact == 0, what
                    assert np.array_equal(rank[rows], ref_rank[rows]), what
                    assert np.array_equal(arg[rows], ref_arg[rows]), what
                    rest = np.setdiff1d(np.arange(n1), rows)
                    assert np.all(rank[rest] == -7) and np.all(arg[rest] == -7), what
    print("rank kernels d %d nc %d: exact on both strips; max(list length / capacity) = %.4f" % (d, nc, worst))


def _falling_table(seed):
    """one query row and 5,000 candidates of width 8 on a cloud ~1,000 steps wide in distance (a few hundred candidates inside
    the gold's window, a handful near the minimum); two candidates carry the range's ends"""
    rng = np.random.RandomState(seed)
    nc, d = 5000, 8
    point = lambda n: (GRID_LO + (40000 + np.round(rng.rand(n, d) * 300 * 256) / 256) * GRID_STEP).astype(F32)
    e1, e2 = point(1), point(nc)
    e2[0, 0], e2[1, 1] = GRID_LO, GRID_LO + 65535 * GRID_STEP
    return e1, e2, d, nc


@pytest.mark.parametrize("kernel", ["plain", "csls"])
def test_rank_kernels_reread_the_row_when_the_running_list_overflows(ops, kernel):
    """candidates ordered so that EVERY column is a record of its thread's running extreme (grid distance falling along the row;
    for CSLS the upper bound rising): the first pass counts 5,000 > kGridTop records, the row is read again against the row's
    extreme and the few columns within the band remain -- n_exact_rows == 0 and the answers are the all-pairs fp64 ones."""
    e1, e2, d, nc = _falling_table(seed=5)
    lo, step = GRID_LO, GRID_STEP
    err = float(F32((d * 1.02 + 1.0) * step))
    G = grid_sums(quantize_ref(e1, lo, 1.0 / step), quantize_ref(e2, lo, 1.0 / step))
    rng = np.random.RandomState(6)
    r = rng.uniform(0.0, 0.3, 1).astype(F32)
    c = rng.uniform(0.0, 0.3, nc).astype(F32)
    if kernel == "plain":
        order = np.argsort(-G[0], kind="stable")
    else:
        order = np.argsort(csls_bounds(G, r, c, step, err)[1][0], kind="stable")
    e2, c, G = e2[order], c[order], G[:, order]
    g = nc // 2
    gold = np.array([g])
    d64 = seq_l1(e1, e2)
    s = sim32(d64)
    if kernel == "plain":
        v, csls = s, None
        Gf = G[0].astype(F32)
        band = (F32(2.0) * plain_tol(s[:, g], step, err)[1] / F32(step))[0]
        records = first_pass_records(nc, lambda j, run: Gf[j] <= run + band, lambda j, run: Gf[j] if run is None else min(run, Gf[j]))
        namb, ntop = plain_counts(G, gold, s[:, g], step, err)
    else:
        v = (F32(2.0) * s - r[:, None]) - c[None, :]
        csls = (ops.to_vec(r), ops.to_vec(c))
        lower, upper = csls_bounds(G, r, c, step, err)
        lower, upper = lower[0], upper[0]
        records = first_pass_records(nc, lambda j, run: upper[j] >= run, lambda j, run: lower[j] if run is None else max(run, lower[j]))
        namb, ntop = csls_counts(G, gold, v[:, g], r, c, step, err)
    assert records > K_TOP, records                                  # the first pass overflows: the re-read has to run
    assert 0 < namb[0] < K_AMB and 0 < ntop[0] < K_TOP, (namb, ntop)  # and leaves lists that fit
    t1, t2 = _table(ops, e1, ld=12), _table(ops, e2)
    grid = ops.L1Grid(t1, t2, d)
    assert grid.step == step and float(F32(grid.err)) == err
    strip = grid.strip(0, 1)
    assert np.array_equal(-strip.cpu().numpy()[:, :nc], G.astype(F32))
    ref_rank, ref_arg = ref_rank_argmax(v, gold)
    for fill in FILLS:
        rank, arg, n_exact = _run_rank(ops, strip, nc, fill, [(0, 1)], t1, t2, d, g, step, grid.err, csls)
        assert n_exact == 0, fill
        assert rank[0] == ref_rank[0] and arg[0] == ref_arg[0], (fill, rank, ref_rank, arg, ref_arg)
    print("rank kernel %s, falling strip: %d first-pass records of %d; re-read keeps %d: max(list length / capacity) = %.4f"
          % (kernel, records, K_TOP, ntop[0], max(namb[0] / K_AMB, ntop[0] / K_TOP)))


# ---------------------------------------------------------------------------------------------
# 6. no silent fallback: the certified lists redo exactly the rows the restatement says
# ---------------------------------------------------------------------------------------------
def _cert_tables(cluster, seed=3):
    rng = np.random.RandomState(seed)
    nq, nc, d = 600, 1031, 75
    tab = (rng.standard_normal((nc, d)) * 0.3).astype(F32)
    if cluster:
        tab[400:520] = tab[400] + 2e-4 * rng.standard_normal((120, d)).astype(F32)     # 120 rows within the grid's error of each other
    q = tab[rng.choice(nc, nq, replace=False)] + 0.01 * rng.standard_normal((nq, d)).astype(F32)
    return q.astype(F32), tab, d


@pytest.mark.parametrize("cluster", [True, False])
def test_certified_lists_fall_back_exactly_where_the_restatement_says(ops, cluster):
    """ops.l1_grid_topk_means and get_neg on a 600 x 1,031 x 75 table: the number of rows sent to the all-pairs fallback == the
    count of a numpy restatement of the certificate (the strip is integer-exact and the exact values bit-exact, so the count is
    determined): 0 on a well-spread table, > 0 and < half the rows on one with a tight cluster of 120; the answers are the
    all-pairs ones either way."""
    from openea_amd.approaches.rdgcn import get_neg
    q, tab, d = _cert_tables(cluster)
    k, margin = 10, 32
    tq, tt = _table(ops, q), _table(ops, tab)
    # ---- l1_grid_topk_means
    grid = ops.L1Grid(tq, tt, d)
    lo = min(float(q.min()), float(tab.min()))
    Gq = grid_sums(quantize_ref(q, lo, 1.0 / grid.step), quantize_ref(tab, lo, 1.0 / grid.step))
    sims = sim32(seq_l1(q, tab))
    bad = restate_topk_means_uncertified(Gq, sims, k, margin, grid.step, grid.err)
    stats = {}
    means = ops.l1_grid_topk_means(tq, tt, grid.q1, grid.q2, d, k, grid.step, grid.err, margin=margin, stats=stats)
    assert stats["uncertified"] == int(bad.sum()), (stats, int(bad.sum()))
    ref_means = ops.row_topk_mean(ops.sim_matrix(tq, tt, d, "manhattan"), k)
    assert torch.equal(means, ref_means)
    # ---- get_neg: the seeds are rows of the table itself
    rng = np.random.RandomState(4)
    seeds = rng.choice(tab.shape[0], 600, replace=False).astype(np.int32)
    lo, hi = float(tab.min()), float(tab.max())
    step = max(hi - lo, 1e-30) / 65535.0
    qt = quantize_ref(tab, lo, 1.0 / step)
    bad_neg, gap = restate_get_neg_uncertified(grid_sums(qt[seeds], qt), tab, seeds, d, k, margin, step)
    assert gap > 1e-9                                               # no seed sits on the edge of its certificate
    stats_neg = {}
    neg = get_neg(ops.to_ids(seeds), tt, d, k, margin=margin, prefilter="u16", stats=stats_neg)
    assert stats_neg["uncertified"] == int(bad_neg.sum()), (stats_neg, int(bad_neg.sum()))
    assert torch.equal(neg, get_neg(ops.to_ids(seeds), tt, d, k, exact_strip=True))
    for n_bad in (int(bad.sum()), int(bad_neg.sum())):
        assert (0 < n_bad < 300) if cluster else n_bad == 0, n_bad
    print("certified lists (%s): topk_means redo %d rows, get_neg %d seeds: max(measured / bound) = equal / equal"
          % ("cluster" if cluster else "spread", int(bad.sum()), int(bad_neg.sum())))


# ---------------------------------------------------------------------------------------------
# 7. row_rank_select with NaN and +-inf
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("n,nc,k", [(300, 42, 10), (257, 157, 125), (5, 1, 1), (64, 1024, 37), (100, 65, 65), (3, 1024, 32)])
def test_row_rank_select_gives_nan_a_place_and_stays_in_its_slots(ops, dtype, n, nc, k, largest):
    """oea_row_rank_select_* on rows holding 0, 1, k, nc - k + 1 and nc NaNs, +-inf and ties: the selection and the k-th value ==
    a stable numpy sort (NaN last in both directions, NaNs among themselves by column), every row writes its k slots and nothing
    else -- out_sel is n k + nc ints pre-filled with -1 (room for the overrun of a kernel that ranks every NaN first), and every
    slot past n k must still hold -1."""
    rng = np.random.RandomState(n + nc + k)
    np_t = F32 if dtype == "f32" else np.float64
    v = rng.standard_normal((n, nc))
    v[:, ::3] = np.round(v[:, ::3], 1)                               # ties
    v = v.astype(np_t)
    for row in range(n):
        if nc > 2 and row % 2:
            at = rng.choice(nc, 2, replace=False)
            v[row, at[0]], v[row, at[1]] = np.inf, -np.inf
        if nc > 8 and row % 4 == 3:
            v[row, rng.choice(nc, 3, replace=False)] = np.inf if row % 8 == 3 else -np.inf     # tied infinities
        m = min((0, 1, k, nc - k + 1, nc)[row % 5], nc)
        v[row, rng.choice(nc, m, replace=False)] = np.nan
    ids = np.sort(rng.choice(100000, (n, nc), replace=True), axis=1).astype(np.int32)
    dev = ops.device()
    dv, dids = torch.from_numpy(v).to(dev), torch.from_numpy(ids).to(dev)
    order = np.argsort(-v if largest else v, axis=1, kind="stable")[:, :k]       # numpy sorts NaN (and -NaN) last
    cols = np.sort(order, axis=1)
    ref_kth = np.take_along_axis(v, order[:, k - 1:k], 1).reshape(-1)
    fn = ops.lib().oea_row_rank_select_f32 if dtype == "f32" else ops.lib().oea_row_rank_select_f64
    for use_ids in (True, False):
        sel = torch.full((n * k + nc,), -1, dtype=torch.int32, device=dev)
        kth = torch.full((n,), 777.0, dtype=dv.dtype, device=dev)
        ops.check(fn(ops._p(dv), n, nc, nc, k, int(largest), ops._p(dids) if use_ids else None, nc if use_ids else 0, ops._p(sel),
                     ops._p(kth), ops._stream()))
        sel = sel.cpu().numpy()
        assert np.all(sel[n * k:] == -1)                             # nothing past the last row's k slots
        want = np.take_along_axis(ids, cols, 1) if use_ids else cols
        assert np.array_equal(sel[:n * k].reshape(n, k), want), np.argwhere(sel[:n * k].reshape(n, k) != want)[:4]
        assert np.array_equal(kth.cpu().numpy(), ref_kth, equal_nan=True)
    print("row_rank_select %s n %d nc %d k %d largest %d: max(measured / bound) = 0 (equal to the stable sort)"
          % (dtype, n, nc, k, largest))
