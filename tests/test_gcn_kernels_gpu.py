"""GPU parity tests of csrc/spmm.hip: the CSR aggregate (short-row, workgroup-cooperative and hub-chunk / ticket paths), the L1
alignment hinge (workgroup-per-link and lane-group-per-link kernels, atomic and coefficient mode) and the row SGD step through the
L2 normalisation, each against an fp64 restatement at the shapes the kernels branch on.

Every buffer a kernel stores to is pre-filled with NaN (the atomic gradient, which accumulates, with the zeros it requires), so a
row that is never stored fails its comparison.  Every bound below is derived from the operation count and the fp32 unit roundoff
U = 2^-24, and written next to its assert; each test prints max(err / bound)."""
import ctypes as C
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

U = 2.0 ** -24                      # fp32 unit roundoff
K_LONG = 96                         # spmm.hip kLongRow: rows up to here are summed serially in CSR order
THRESH, CHUNK = 200, 128            # the split of the hub rows used throughout (as tests/test_kernels_gpu.py::test_spmm_bit_exact)
PAD = 7.0                           # finite sentinel in the padding columns of x and mask_from
WIDTHS = [1, 30, 64, 75, 100, 130, 200, 300, 500, 1200]


@pytest.fixture(scope="module")
def ops():
    from openea_amd import ops as _ops
    _ops.lib()   # raises loudly if the HIP library / GPU is missing
    return _ops


def _pad4(d):
    return (d + 3) // 4 * 4


def _bits(t):
    return t.contiguous().view(torch.int32)


def _nan(shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


# ---------------------------------------------------------------------------------------------
# 1. the aggregate
# ---------------------------------------------------------------------------------------------
def _agg_ng(ld):
    """rows per workgroup of spmm_csr_kernel: 16-lane groups up to ld = 128, 64-lane groups above"""
    return 16 if ld <= 128 else 4


HUB_LENS = [THRESH + 1, 2 * CHUNK, 2 * CHUNK + 1, 5 * CHUNK + 17]         # the four split rows
PINNED_LENS = [0, 1, 3, 4, 5, 63, 64, 65, K_LONG, K_LONG + 1, 111, 112, 113, THRESH] + HUB_LENS


class _Graph:
    """a CSR built by hand: chosen row lengths, random column ids (repeats allowed, unsorted), random fp32 values of both signs"""

    def __init__(self, lens, n_cols, seed):
        rng = np.random.RandomState(seed)
        self.lens = np.asarray(lens, np.int64)
        self.n_rows, self.n_cols = len(self.lens), n_cols
        self.indptr = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)
        nnz = int(self.indptr[-1])
        self.indices = rng.randint(0, n_cols, nnz).astype(np.int32)
        self.vals = rng.standard_normal(nnz).astype(np.float32)
        self.rows = np.repeat(np.arange(self.n_rows), self.lens).astype(np.int32)
        self._dev = None
        self._cases = {}

    def dev(self, ops):
        if self._dev is None:
            self._dev = (ops.to_ids(self.indptr), ops.to_ids(self.indices), ops.to_vec(self.vals))
        return self._dev

    def split(self, ops, row_range=None):
        return ops.csr_split(self.indptr, threshold=THRESH, chunk=CHUNK, row_range=row_range)

    def case(self, d, seed=0):
        """inputs of width d and their references, computed once per (graph, d, seed) and shared: x and mask_from (host
        [*, ld], padding columns = PAD), ref64 = the fp64 product of the same fp32 inputs, mag = sum_e |v_e| |x[c_e, j]| (fp64),
        ref32 = the C oracle's serial fp32 fmaf sum in CSR order"""
        key = (d, seed)
        if key not in self._cases:
            import scipy.sparse as sp
            from oracle import cport
            rng = np.random.RandomState(1000 * d + seed)
            ld = _pad4(d)
            x = np.full((self.n_cols, ld), PAD, np.float32)
            x[:, :d] = rng.standard_normal((self.n_cols, d)).astype(np.float32)
            mask = np.full((self.n_rows, ld), PAD, np.float32)
            m = rng.standard_normal((self.n_rows, d)).astype(np.float32)
            u = rng.rand(self.n_rows, d)
            m[u < 0.1] = 0.0                          # the gate is strictly > 0: zeros of both signs close it
            m[u > 0.9] = -0.0
            mask[:, :d] = m
            shape = (self.n_rows, self.n_cols)
            a64 = sp.csr_matrix((self.vals.astype(np.float64), self.indices, self.indptr), shape=shape)
            abs64 = sp.csr_matrix((np.abs(self.vals).astype(np.float64), self.indices, self.indptr), shape=shape)
            x64 = x[:, :d].astype(np.float64)
            c = types.SimpleNamespace(d=d, ld=ld, x=x, mask=mask, ref64=np.asarray(a64 @ x64), mag=np.asarray(abs64 @ np.abs(x64)),
                                      ref32=cport.spmm_coo(self.rows, self.indices, self.vals, np.ascontiguousarray(x[:, :d]), self.n_rows))
            self._cases[key] = c
        return self._cases[key]


_GRAPHS = {}


def _main_graph():
    """~300 rows holding every length the kernel branches on, positions shuffled (hubs not all at the low ids)"""
    if "main" not in _GRAPHS:
        rng = np.random.RandomState(7)
        fill = rng.randint(0, 13, 300 - len(PINNED_LENS))
        _GRAPHS["main"] = _Graph(rng.permutation(np.concatenate([PINNED_LENS, fill])), 300, seed=11)
    return _GRAPHS["main"]


def _small_graph(name, lens):
    if name not in _GRAPHS:
        _GRAPHS[name] = _Graph(lens, 50, seed=13 + len(lens))
    return _GRAPHS[name]


def _expected(c, act, masked, ref):
    e = ref
    if act:
        e = np.maximum(e, 0)
    if masked:
        e = e * (c.mask[:, :c.d] > 0)
    return e


def _check_aggregate(got, g, c, act, masked, tag, rows=None):
    """got: host [n_rows, ld].  fp64 bound on every element, short rows bit-equal to the serial oracle, padding and empty rows 0."""
    sl = slice(None) if rows is None else slice(*rows)
    d = c.d
    got = got[sl]
    lens = g.lens[sl]
    exp64 = _expected(c, act, masked, c.ref64)[sl]
    err = np.abs(got[:, :d].astype(np.float64) - exp64)
    # the standard bound for an fp32 FMA sum of nnz terms in ANY order (serial, strided per group, partials combined per group and
    # per chunk): nnz U sum |v x| to first order; the + 4 covers the second-order terms.  relu is 1-Lipschitz and the gate
    # multiplies by 0 / 1, so the same bound holds after them.
    bound = (lens[:, None] + 4) * U * c.mag[sl]
    pos = bound > 0
    ratio = float(np.max(err[pos] / bound[pos])) if pos.any() else 0.0
    print("aggregate %s d=%d: max err/bound = %.4f" % (tag, d, ratio))
    assert np.isfinite(got).all(), "%s: a row was never stored" % tag
    assert (err <= bound).all(), "%s: fp64 bound missed, max err/bound %.3f" % (tag, ratio)
    short = lens <= K_LONG
    assert np.array_equal(got[short][:, :d], _expected(c, act, masked, c.ref32)[sl][short]), "%s: short rows not bit-equal" % tag
    assert (got[:, d:] == 0).all(), "%s: padding columns not exactly 0" % tag
    assert (got[lens == 0] == 0).all(), "%s: empty rows not exactly 0" % tag


def _run_modes(ops, g, d):
    """plain; relu; relu + mask_from + hub split -- each into a NaN-filled output"""
    c = g.case(d)
    rowptr, colidx, vals = g.dev(ops)
    x, mask = ops.to_table(c.x, ld=c.ld), ops.to_table(c.mask, ld=c.ld)
    dev = x.device
    y = ops.spmm_csr(rowptr, colidx, vals, x, d, out=_nan((g.n_rows, c.ld), dev))
    _check_aggregate(y.cpu().numpy(), g, c, 0, False, "plain")
    y = ops.spmm_csr(rowptr, colidx, vals, x, d, act=1, out=_nan((g.n_rows, c.ld), dev))
    _check_aggregate(y.cpu().numpy(), g, c, 1, False, "relu")
    split = g.split(ops)
    y = ops.spmm_csr(rowptr, colidx, vals, x, d, act=1, mask_from=mask, out=_nan((g.n_rows, c.ld), dev), split=split)
    _check_aggregate(y.cpu().numpy(), g, c, 1, True, "relu+mask+split")
    if split is not None:
        assert int(split._keep[-1].abs().sum()) == 0, "tickets not reset"
    return split


@pytest.mark.parametrize("d", WIDTHS)
def test_aggregate_pinned_row_lengths_vs_fp64(ops, d):
    g = _main_graph()
    assert set(PINNED_LENS) <= set(g.lens.tolist())
    split = _run_modes(ops, g, d)
    assert split.n_rows == len(HUB_LENS) and split.n_chunks == 2 + 2 + 3 + 6      # 201, 256, 257, 657 edges in chunks of 128


@pytest.mark.parametrize("d", WIDTHS)
def test_aggregate_one_row_and_one_row_more_than_a_workgroup(ops, d):
    for i, n_edges in enumerate([5, 113, 2 * CHUNK + 1]):                         # n_rows = 1: short, cooperative, split
        _run_modes(ops, _small_graph("one%d" % i, [n_edges]), d)
    ng = _agg_ng(_pad4(d))
    pattern = [K_LONG + 1, 0, THRESH + 1, 5, 2 * CHUNK + 1, 1, K_LONG, 113, 0, 64, 4, THRESH, 3, 65, 2 * CHUNK, 63, 112]
    _run_modes(ops, _small_graph("ng%d" % ng, pattern[:ng + 1]), d)              # n_rows = NG + 1: the second workgroup has one row


# ---------------------------------------------------------------------------------------------
# 2. the split operand: repeated launches, row ranges, the two other epilogues
# ---------------------------------------------------------------------------------------------
def _split_launch(ops, g, split, d, seed, rows=None, out=None):
    c = g.case(d, seed)
    rowptr, colidx, vals = g.dev(ops)
    x, mask = ops.to_table(c.x, ld=c.ld), ops.to_table(c.mask, ld=c.ld)
    if out is None:
        out = _nan((g.n_rows, c.ld), x.device)
    if rows is None:
        ops.spmm_csr(rowptr, colidx, vals, x, d, act=1, mask_from=mask, out=out, split=split)
    else:                                        # exactly as models/graph_ops.py:CsrOperand.apply drives a rank's block
        lo, hi = rows
        ops.spmm_csr(rowptr[lo: hi + 1], colidx, vals, x, d, act=1, mask_from=mask[lo:hi], out=out[lo:hi], split=split)
    return out, c


def test_split_operand_relaunched_at_other_widths(ops):
    g = _main_graph()
    split = g.split(ops)
    tickets = split._keep[-1]
    sizes = []
    for d, seed in ((62, 1), (299, 2), (61, 3)):            # ld = 64, 300 (the partials buffer grows), 64 again: a different x each
        out, c = _split_launch(ops, g, split, d, seed)
        assert int(tickets.abs().sum()) == 0, "tickets not reset after the launch at d=%d" % d
        sizes.append(int(split.partials_floats))
        _check_aggregate(out.cpu().numpy(), g, c, 1, True, "relaunch d=%d" % d)
    assert sizes == [split.n_chunks * 64, split.n_chunks * 300, split.n_chunks * 300]
    first, c = _split_launch(ops, g, split, 299, 2)
    for _ in range(2):                                       # the bits do not depend on which chunk finishes last
        again, _ = _split_launch(ops, g, split, 299, 2)
        assert int(tickets.abs().sum()) == 0
        assert torch.equal(_bits(first), _bits(again))
    _check_aggregate(first.cpu().numpy(), g, c, 1, True, "relaunch d=299 again")


@pytest.mark.parametrize("d", [75, 300])
def test_split_of_a_row_range_equals_the_unsharded_rows(ops, d):
    g = _main_graph()
    hubs = np.flatnonzero(g.lens > THRESH)
    lo, hi = int(hubs[0]) + 1, int(hubs[-1])                # the first and the last hub row lie outside, the two others inside
    assert lo > 0 and ((hubs >= lo) & (hubs < hi)).sum() == 2 and (g.lens[lo:hi] > K_LONG).sum() > 2
    full, c = _split_launch(ops, g, g.split(ops), d, 4)
    part = g.split(ops, row_range=(lo, hi))
    assert part.n_rows == 2
    out, _ = _split_launch(ops, g, part, d, 4, rows=(lo, hi))
    assert torch.equal(_bits(out[lo:hi]), _bits(full[lo:hi]))
    assert bool(torch.isnan(out[:lo]).all()) and bool(torch.isnan(out[hi:]).all()), "rows outside the range were written"
    assert int(part._keep[-1].abs().sum()) == 0
    _check_aggregate(out.cpu().numpy(), g, c, 1, True, "row_range", rows=(lo, hi))


@pytest.mark.parametrize("d", [30, 75, 130, 300, 1200])
def test_split_epilogues_without_tickets_and_without_partials(ops, d):
    g = _main_graph()
    ticket_path, c = _split_launch(ops, g, g.split(ops), d, 5)
    # partials, no tickets: every workgroup leaves its chunk sum, spmm_rows_epilogue_kernel adds them in chunk order = the same bits
    no_tickets = g.split(ops)
    no_tickets.tickets = None
    out, _ = _split_launch(ops, g, no_tickets, d, 5)
    assert torch.equal(_bits(out), _bits(ticket_path))
    # no partials: zeroed hub rows + fp32 atomics per chunk + epilogue (a direct call: ops.spmm_csr would attach a buffer)
    legacy = g.split(ops)
    assert not legacy.partials and legacy.partials_floats == 0
    rowptr, colidx, vals = g.dev(ops)
    x, mask = ops.to_table(c.x, ld=c.ld), ops.to_table(c.mask, ld=c.ld)
    out = _nan((g.n_rows, c.ld), x.device)
    ops.check(ops.lib().oea_spmm_csr(ops._p(rowptr), ops._p(colidx), ops._p(vals), g.n_rows, ops._p(x), d, c.ld, 1, ops._p(mask),
                                     ops._p(out), c.ld, C.byref(legacy), ops._stream()))
    _check_aggregate(out.cpu().numpy(), g, c, 1, True, "atomic chunks")
    short = torch.from_numpy(g.lens <= THRESH).to(out.device)
    assert torch.equal(_bits(out[short]), _bits(ticket_path[short]))


# ---------------------------------------------------------------------------------------------
# 3. the L1 hinge
# ---------------------------------------------------------------------------------------------
GAMMA = 3.0 + 2.0 ** -7            # a multiple of 2^-6 plus 2^-7: no hinge value is 0


def _scale32(k, t):
    """as the kernels form it"""
    return np.float32(1) / (np.float32(2) * np.float32(k) * np.float32(t))


def _hinge_inputs(n, t, k, d, form, seed):
    """embeddings on the 2^-6 grid in [-4, 4] (every |difference| sum is exact in fp32 in any order up to ld = 1280), zero
    padding, planted exact-zero differences; links; the production or the adversarial negative lists"""
    rng = np.random.RandomState(seed)
    ld = _pad4(d)
    emb = np.zeros((n, ld), np.float32)
    emb[:, :d] = rng.randint(-256, 257, (n, d)).astype(np.float32) / 64.0
    l = rng.randint(0, n, t)
    if form == "adversarial":
        l[:5] = l[0]                                                  # an entity in many links
    r = (l + 1 + rng.randint(0, n - 1, t)) % n                        # r != l
    L_, R_ = np.repeat(l, k), np.repeat(r, k)
    m = t * k
    nl, nr = L_.copy(), rng.randint(0, n, m)                          # gcn_align.py:740-755: neg_left = repeat(l), neg_right random
    n2l, n2r = rng.randint(0, n, m), R_.copy()                        #                       neg2_right = repeat(r), neg2_left random
    if form == "adversarial":
        a_idx, b_idx = np.repeat(np.arange(t), k), np.tile(np.arange(k), t)
        hub = np.full(m, l[0])
        for side, (pl, pr) in enumerate(((nl, nr), (n2l, n2r))):
            rnd = rng.randint(0, n, m)
            foreign = []
            for _ in range(2):
                f = rng.randint(0, n, m)
                for _ in range(3):                                    # two forbidden values: three shifts clear them
                    bad = (f == L_) | (f == R_)
                    f[bad] = (f[bad] + 1) % n
                assert not ((f == L_) | (f == R_)).any()
                foreign.append(f)
            f1, f2 = foreign
            prod = (L_, rnd) if side == 0 else (rnd, R_)
            #           positive pair  swapped    nl == nr    foreign   hub entity  production  nl == r    nr == l
            left = [L_, R_, rnd, f1, hub, prod[0], R_, f1]
            right = [R_, L_, rnd, f2, f1, prod[1], f2, L_]
            pat = (a_idx + b_idx + 3 * side) % 8
            pl[:] = np.choose(pat, left)
            pr[:] = np.choose(pat, right)
    run = max(1, d // 3)
    for a in range(0, t, 4)[:10]:                                     # sgn(0) = 0: a link's rows share a run of columns ...
        emb[r[a], 1:1 + run] = emb[l[a], 1:1 + run]
    for s in range(0, m, 7)[:10]:                                     # ... and so do the rows of some negative pairs
        if nl[s] != nr[s]:
            emb[nr[s], d - run:d] = emb[nl[s], d - run:d]
    ill = np.stack([l, r], 1).astype(np.int32)
    return emb, ill, tuple(np.ascontiguousarray(v, dtype=np.int32) for v in (nl, nr, n2l, n2r))


def _hinge_reference(emb, d, ill, k, negs):
    """fp64 (exact on the grid): L [t, 2k] (i < k: the neg_left / neg_right list, i >= k: neg2_*), per element the sum of the
    gradient's |terms| (unscaled) and per row the number of active pair slots that touch it"""
    e = emb[:, :d].astype(np.float64)
    n, t = e.shape[0], ill.shape[0]
    l, r = ill[:, 0].astype(np.int64), ill[:, 1].astype(np.int64)
    nl_all = np.concatenate([negs[0].reshape(t, k), negs[2].reshape(t, k)], 1).astype(np.int64)
    nr_all = np.concatenate([negs[1].reshape(t, k), negs[3].reshape(t, k)], 1).astype(np.int64)
    dpos = e[l] - e[r]
    A = np.abs(dpos).sum(1)
    B = np.empty((t, 2 * k))
    S = np.zeros((n, d))
    slots = np.zeros(n)
    zero_neg = 0
    step = max(1, (1 << 22) // (2 * k * d))                           # links per block: keeps [links, 2k, d] small
    L = np.empty((t, 2 * k))
    for a0 in range(0, t, step):
        a1 = min(a0 + step, t)
        dneg = e[nl_all[a0:a1]] - e[nr_all[a0:a1]]
        B[a0:a1] = np.abs(dneg).sum(2)
        L[a0:a1] = (A[a0:a1] + GAMMA)[:, None] - B[a0:a1]
        act = L[a0:a1] > 0
        sg = np.abs(np.sign(dneg[act]))
        zero_neg += int((sg == 0).sum())
        np.add.at(S, nl_all[a0:a1][act], sg)
        np.add.at(S, nr_all[a0:a1][act], sg)
        np.add.at(slots, nl_all[a0:a1][act], 1)
        np.add.at(slots, nr_all[a0:a1][act], 1)
    act = L > 0
    cnt = act.sum(1)
    sp = np.abs(np.sign(dpos)) * cnt[:, None]
    np.add.at(S, l, sp)
    np.add.at(S, r, sp)
    np.add.at(slots, l, cnt > 0)
    np.add.at(slots, r, cnt > 0)
    assert (L != 0).all()
    assert (dpos == 0).any() and zero_neg > 0, "no exact-zero difference planted"
    return L, act, cnt, S, slots


def _check_hinge(ops, n, t, k, d, form, seed, exact_grad=False):
    from oracle import np_oracle
    emb, ill, negs = _hinge_inputs(n, t, k, d, form, seed)
    ld = emb.shape[1]
    L, act, cnt, S, slots = _hinge_reference(emb, d, ill, k, negs)
    assert act.any() and not act.all()
    scale = _scale32(k, t)
    loss_o, g64 = np_oracle.align_loss_and_grad(emb[:, :d], ill, GAMMA, k, *negs)
    sum_l = float(L[act].sum())                                       # exact: multiples of 2^-7 far below 2^53
    assert abs(loss_o - sum_l / (2.0 * k * t)) <= 1e-12 * abs(loss_o)
    loss_ref = sum_l * float(scale)
    emb_d, ill_d = ops.to_table(emb, ld=ld), ops.to_ids(ill)
    negs_d = tuple(ops.to_ids(v) for v in negs)
    dev = emb_d.device
    tag = "hinge %s n=%d t=%d k=%d d=%d" % (form, n, t, k, d)

    # coefficient mode: every pair's coefficient, bit for bit
    coef = _nan((t + 2 * t * k,), dev)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    ops.align_loss_l1_coef(emb_d, d, ill_d, k, GAMMA, *negs_d, loss, coef)
    coef_h = coef.cpu().numpy()
    coef_ref = np.concatenate([scale * cnt.astype(np.float32), np.where(act.reshape(-1), -scale, np.float32(0))]).astype(np.float32)
    assert np.array_equal(coef_h[:t].view(np.uint32), coef_ref[:t].view(np.uint32)), tag + ": link coefficients"
    assert np.array_equal(coef_h[t:].view(np.uint32), coef_ref[t:].view(np.uint32)), tag + ": active set / negative coefficients"
    assert abs(float(loss.item()) - loss_ref) <= 1e-12 * abs(loss_ref), tag + ": loss (coefficient mode)"

    # the two gradients
    grad_a = torch.zeros((n, ld), dtype=torch.float32, device=dev)     # accumulated into: the zeros are required
    loss_a = torch.zeros(1, dtype=torch.float64, device=dev)
    ops.align_loss_l1(emb_d, d, ill_d, k, GAMMA, *negs_d, grad_a, loss_a)
    assert abs(float(loss_a.item()) - loss_ref) <= 1e-12 * abs(loss_ref), tag + ": loss (atomic mode)"
    nl, nr, n2l, n2r = negs_d                                          # as approaches/gcn_align.py:_pair_lists builds them
    neg_pairs = torch.stack([torch.stack([nl.view(t, k), n2l.view(t, k)], 1).reshape(-1),
                             torch.stack([nr.view(t, k), n2r.view(t, k)], 1).reshape(-1)], 1)
    csr = ops.pair_rows_csr(torch.cat([ill_d.to(neg_pairs.dtype), neg_pairs]), n)
    grad_c = ops.pair_grad_rows(emb_d, d, *csr, coef, norm=1, out=_nan((n, ld), dev))
    # m terms of one row element, each scale * (an integer) rounded once, added in fp32 in any order: (m - 1) + 1 roundings, + 1
    # for scale32 against the reference's fp64 1 / (2 k t)
    bound = (slots[:, None] + 2) * U * S / (2.0 * k * t)
    for name, g in (("atomic", grad_a), ("composed", grad_c)):
        gh = g.cpu().numpy()
        err = np.abs(gh[:, :d].astype(np.float64) - g64)
        pos = bound > 0
        ratio = float(np.max(err[pos] / bound[pos]))
        print("%s %s gradient: max err/bound = %.4f" % (tag, name, ratio))
        assert np.isfinite(gh).all(), "%s %s: a row was never stored" % (tag, name)
        assert (err <= bound).all(), "%s %s gradient: max err/bound %.3f" % (tag, name, ratio)
        assert (gh[:, d:] == 0).all(), "%s %s: padding columns" % (tag, name)
        if exact_grad:                                                 # 1 / (2 k t) is a power of two: every term and sum is exact
            assert np.array_equal(gh[:, :d], g64.astype(np.float32)), "%s %s gradient not bit-equal" % (tag, name)


# (d, k): align_coef_groups_kernel IT 1..4 (ld <= 32 / 64 / 96 / 128 with k <= 16); align_loss_l1_kernel (32,1) (32,2) (32,3) (32,4)
# (64,4) (64,8) (64,20) in the atomic mode (any k) and in the coefficient mode (k > 16 or ld > 128); k = 16 | 17 at ld <= 128 and
# ld = 128 | 132 at k = 16 cross between the two kernels; k = 1: 2k < NG; (300, 125): RDGCN's shape
HINGE_CASES = [(8, 1), (8, 17), (30, 5), (30, 125), (33, 16), (33, 17), (75, 5), (75, 17), (100, 5), (128, 16), (128, 17), (130, 16),
               (130, 1), (300, 5), (300, 125), (1200, 5), (1200, 17)]


@pytest.mark.parametrize("form", ["production", "adversarial"])
@pytest.mark.parametrize("d,k", HINGE_CASES)
def test_l1_hinge_exact_on_a_grid(ops, d, k, form):
    _check_hinge(ops, 200, 37, k, d, form, seed=100 * d + k)


@pytest.mark.parametrize("form", ["production", "adversarial"])
def test_l1_hinge_second_grid_trip(ops, form):
    """t = 66,000 > 65,535 workgroups of align_loss_l1_kernel and > 4,096 x 8 lane groups of align_coef_groups_kernel"""
    _check_hinge(ops, 64, 66000, 1, 8, form, seed=5)


@pytest.mark.parametrize("form", ["production", "adversarial"])
@pytest.mark.parametrize("d", [100, 130])
def test_l1_hinge_gradient_bit_exact_when_the_scale_is_a_power_of_two(ops, d, form):
    """t = 32, k = 16: 1 / (2 k t) = 2^-10 (d = 100: the lane-group kernel writes the coefficients, d = 130: the workgroup kernel)"""
    _check_hinge(ops, 200, 32, 16, d, form, seed=9 + d, exact_grad=True)


# ---------------------------------------------------------------------------------------------
# 4. row SGD through the normalisation
# ---------------------------------------------------------------------------------------------
def _sgd_ng(ld):
    """rows per workgroup of sgd_rows_kernel (OEA_DISPATCH_LD)"""
    return 16 if ld <= 64 else 8 if ld <= 128 else 4


def _check_sgd(ops, w, g, d, normalize, lr, tag):
    ld = _pad4(d)
    wd = ops.sgd_rows_(ops.to_table(w), ops.to_table(g), d, normalize, lr)
    got = wd.cpu().numpy()
    lr = float(np.float32(lr))
    w64, g64 = w.astype(np.float64), g.astype(np.float64)
    if normalize:                                      # oracle/np_oracle.py:gcn_se_epoch
        inv = 1.0 / np.sqrt(np.maximum((w64 ** 2).sum(1, keepdims=True), 1e-12))
        T = w64 * inv
        g_w = (g64 - T * (T * g64).sum(1, keepdims=True)) * inv
        # the sum of squares (ld positive terms, relative error <= ld U) sits under a square root: inv carries ld/2 U, and inv
        # enters the projected term T (T.g) three times (1.5 ld U) next to the ld-term dot product (ld U on sum |T_j g_j|): 2.5 ld U,
        # against 0.5 ld U on the g term.  The + 8 takes rsqrtf's few ulp, the clamp constant in fp32 and the half dozen products
        # and differences of the update.  c = 3 is 2.5 rounded up.
        c = 3.0
        bound = c * (ld + 8) * U * (np.abs(w64) + lr * inv * (np.abs(g64) + np.abs(T) * np.abs(T * g64).sum(1, keepdims=True)))
    else:
        g_w = g64
        bound = 3 * U * (np.abs(w64) + lr * np.abs(g64))              # w - lr g: one product, one difference (2 U, + 1 U slack)
    ref = w64 - lr * g_w
    err = np.abs(got[:, :d].astype(np.float64) - ref)
    pos = bound > 0
    ratio = float(np.max(err[pos] / bound[pos])) if pos.any() else 0.0
    print("sgd_rows %s d=%d rows=%d normalize=%d: max err/bound = %.4f" % (tag, d, w.shape[0], normalize, ratio))
    assert np.isfinite(got).all()
    assert (err <= bound).all(), "sgd_rows %s: max err/bound %.3f" % (tag, ratio)
    assert (got[:, d:] == 0).all(), "padding columns of w moved"
    return ref


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("rows", ["1", "NG+1", "257"])
@pytest.mark.parametrize("d", [30, 75, 100, 200, 300, 1200])
def test_sgd_rows_vs_fp64(ops, d, rows, normalize):
    rng = np.random.RandomState(d + (1 if normalize else 0))
    lr = 0.05
    n = {"1": 1, "NG+1": _sgd_ng(_pad4(d)) + 1, "257": 257}[rows]
    w = (0.5 * rng.standard_normal((n, d))).astype(np.float32)        # row norms ~ sqrt(d) / 2: far from 1
    g = rng.standard_normal((n, d)).astype(np.float32)
    tiny = (1e-3 / np.sqrt(d) * rng.standard_normal(d)).astype(np.float32)        # a row of norm ~ 1e-3
    if n == 1:
        _check_sgd(ops, w, g, d, normalize, lr, "plain row")
        ref = _check_sgd(ops, np.zeros((1, d), np.float32), g, d, normalize, lr, "zero row")
        if normalize:
            np.testing.assert_allclose(ref, -float(np.float32(lr)) * g.astype(np.float64) * 1e6, rtol=1e-12)    # the clamp branch
        _check_sgd(ops, tiny[None], g, d, normalize, lr, "tiny row")
        return
    w[n // 2] = 0.0
    w[n - 1] = tiny
    ref = _check_sgd(ops, w, g, d, normalize, lr, "mixed rows")
    if normalize:
        np.testing.assert_allclose(ref[n // 2], -float(np.float32(lr)) * g[n // 2].astype(np.float64) * 1e6, rtol=1e-12)


# ---------------------------------------------------------------------------------------------
# 5. the one-call epoch against the same epoch op by op
# ---------------------------------------------------------------------------------------------
def _epoch_by_ops(ops, unit, negs):
    """the world > 1 branch of GCN_Align_Unit.train_step without the exchange"""
    d, k = unit.dim, unit.args.neg_triple_num
    T, H1, out = unit.forward()
    pairs = unit._pair_lists(negs, out.shape[0])
    assert pairs is not None
    coef = ops.align_loss_l1_coef(out, d, unit.ILL, k, unit.args.gamma, *negs, unit.loss)
    g_out = ops.pair_grad_rows(out, d, *pairs, coef, norm=1)
    g_pre1 = unit.adj.tmm(g_out, d, mask_from=H1)
    g_x = unit.adj.tmm(g_pre1, d)
    g_T = g_x if unit.features is None else unit.features.tmm(g_x, d)
    ops.sgd_rows_(unit.W, g_T, d, True, unit.args.learning_rate)
    return out


@pytest.mark.parametrize("kind", ["structure", "attribute"])
@pytest.mark.parametrize("n", [400, 1000])
def test_one_call_epoch_equals_the_epoch_op_by_op(ops, n, kind):
    """n = 400, d = 75, k = 5.  A 400 x 400 support matrix cannot hold a row above the production hub threshold (768 nonzeros
    after sum_duplicates), so at n = 400 the live split is the attribute unit's feature operand (one entity with 800 of 900
    attributes); n = 1000 adds the support matrix with an 800-neighbour hub (its transpose has the hub too).
    t = 8 links: the hinge then runs in ONE workgroup, so the double atomics of the loss have one order and the loss is bit-equal."""
    import scipy.sparse as sp
    from openea_amd.approaches.gcn_align import DeviceCSR, GCN_Align_Unit
    d, k, t, f = 75, 5, 8, 900
    rng = np.random.RandomState(n)
    dev = ops.device()
    rows, cols = np.repeat(np.arange(n), 3), rng.randint(0, n, 3 * n)
    hub_deg = 800 if n > 800 else 300
    rows = np.concatenate([rows, np.full(hub_deg, 137)])
    cols = np.concatenate([cols, rng.permutation(n)[:hub_deg]])
    half = sp.coo_matrix((0.05 + 0.25 * rng.rand(len(rows)), (rows, cols)), shape=(n, n)).tocsr()
    adj = DeviceCSR(half + half.T, dev)
    if n > 800:
        assert adj.fwd.split is not None and adj.bwd.split is not None, "the support's hub split is not live"
    feats = None
    if kind == "attribute":
        fr, fc = np.repeat(np.arange(n), 4), rng.randint(0, f, 4 * n)
        fr = np.concatenate([fr, np.full(800, 211)])
        fc = np.concatenate([fc, rng.permutation(f)[:800]])
        fm = sp.coo_matrix((np.ones(len(fr)), (fr, fc)), shape=(n, f)).tocsr()
        fm.data[:] = 1.0
        feats = DeviceCSR(fm, dev)
        assert feats.fwd.split is not None, "the feature operand's hub split is not live"
    links = rng.permutation(n)[:2 * t].reshape(t, 2)
    args = types.SimpleNamespace(neg_triple_num=k, gamma=3.0, learning_rate=0.1)
    w_rows = n if feats is None else f
    fused = GCN_Align_Unit(args, adj, w_rows, d, links, features=feats, seed=3)
    by_ops = GCN_Align_Unit(args, adj, w_rows, d, links, features=feats, seed=3)
    assert torch.equal(_bits(fused.W), _bits(by_ops.W))
    negs = (ops.to_ids(np.repeat(links[:, 0], k)), ops.to_ids(rng.randint(0, n, t * k)),
            ops.to_ids(rng.randint(0, n, t * k)), ops.to_ids(np.repeat(links[:, 1], k)))
    w0 = fused.W.clone()
    for epoch in range(2):
        fused._train_step_fused(negs)
        out = _epoch_by_ops(ops, by_ops, negs)
        assert torch.equal(_bits(fused.outputs), _bits(out)), "outputs differ in epoch %d" % epoch
        assert torch.equal(_bits(fused.W), _bits(by_ops.W)), "W differs after epoch %d" % epoch
    assert not torch.equal(fused.W, w0) and bool(torch.isfinite(fused.W).all())
    loss_f, loss_o = float(fused.loss.item()), float(by_ops.loss.item())
    assert loss_f > 0 and loss_f == loss_o
