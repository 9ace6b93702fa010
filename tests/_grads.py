"""What test_step_edges_gpu.py holds the fused steps to: problems at edge shapes, their float64 gradients and the tolerances.

Everything here runs on the CPU.  The float64 references are the restatements the suite already has (semantic_grads,
distmult_grads, jape_triple_grads, weighted_pair_loss, the SGD restatement of test_mapping_step_matches_oracle); their float32
runs are the same torch / numpy code on float32 tensors.  A problem is built once per process (functools.lru_cache) and is not
written to afterwards.

The comparison (gradient_check).  A step runs under SGD with lr = 1.0: lr g is exact, so after = fl(before - g) and
before - after, formed in float64 from the float32 bits, is the gradient up to the rounding of `after`: half an ulp of after,
at most 2^-24 |after| per element.  A row of a table passes when

    | (before - after) - g64 |_2  <=  4 E32 + 2^-24 |after row|_2

where g64 is the float64 restatement on the float32-rounded tables and E32 is the largest row L2 deviation, over that table, of
the float32 run of the restatement from its float64 run -- measured from the reference, never from the kernel.  The second term
is exactly the recovery error above.  The factor 4 is the margin test_conve_gpu.py gives over measured fp32 noise.

The loss (loss_check): |loss - loss64| <= (d + 32) 2^-24 sum |term| over the per-triple terms of the float64 loss: a d-term
fp32 dot product (d 2^-24 in the worst order), two row normalisations and the transcendental (a few ulp each, inside the 32)
per term, the terms then summed in double."""
import contextlib
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import test_semantic_cpu as sem  # noqa: E402
from test_iptranse_cpu import _grads as pair_grads, weighted_pair_loss  # noqa: E402
from test_jape_cpu import jape_triple_grads, jape_triple_loss  # noqa: E402
from test_rotate_distmult_cpu import distmult_grads, distmult_loss  # noqa: E402

U24 = 2.0 ** -24
N_ENT, N_REL = 600, 24            # the last 100 entities and the last 4 relations are in no triple
ENT_TAIL, REL_TAIL = 100, 4
NEG_ALPHA = 0.1                   # JAPE
PAIR_MARGIN = 1.5                 # the weighted pair step (test_iptranse_gpu.MARGIN)
PAIR_KINK = 1e-5                  # test_iptranse_gpu.KINK: no float64 hinge argument of a pair lies this close to zero
MODELS = ("HolE", "SimplE", "DistMult", "JAPE", "WPair")


def f32(a):
    """float64 values that float32 holds exactly"""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _xavier(rng, rows, dim):
    from openea_amd.modules.base.initializers import xavier_host
    return f32(xavier_host(rng, (rows, dim)))


# ---- batches -------------------------------------------------------------------------------------------------------------------
def edge_batch(rng, n, k, n_ent=N_ENT, n_rel=N_REL):
    """test_semantic_gpu._zipf_batch (Zipf relations, one entity in many triples, h == t positives, negatives with another
    relation than their positive's) with, in the first negative of the first positives:
      0  a negative identical to its positive,
      1  a negative whose head is its positive's tail (the cross-slot case of row_ops.h's Slots),
      2  a negative that shares no row with its positive (another head, relation and tail),
      3  an h == t positive on the hub entity, its negatives corrupted again,
      4  the hub entity once more (so that n = 5 still has a row with two positives).
    -> pos [n, 3], neg [n k, 3] int32.  A batch shorter than five positives holds what fits."""
    from test_semantic_gpu import _zipf_batch
    used, common = n_ent - ENT_TAIL, n_rel - REL_TAIL
    m = max(n, 64)                                     # _zipf_batch draws 50 distinct negatives for the other relations
    pos, neg = _zipf_batch(rng, n_ent, n_rel, m, k)
    neg = neg.reshape(m, k, 3)
    neg[0, 0] = pos[0]
    neg[1, 0] = (pos[1, 2], pos[1, 1], rng.randint(0, used))
    h, r, t = pos[2]
    free = [e for e in range(used) if e not in (h, t)]
    neg[2, 0] = (free[rng.randint(len(free))], (r + 1 + rng.randint(common - 1)) % common, free[rng.randint(len(free))])
    pos[3, 2] = pos[3, 0] = pos[0, 0]
    neg[3] = pos[3]
    neg[3, np.arange(k), rng.randint(0, 2, k) * 2] = rng.randint(0, used, k)
    pos[4, 0] = pos[0, 0]
    neg[4] = pos[4]
    neg[4, :, 2] = rng.randint(0, used, k)
    pos, neg = pos[:n], neg[:n]
    assert pos[:, [0, 2]].max() < used and neg[:, :, [0, 2]].max() < used and max(pos[:, 1].max(), neg[:, :, 1].max()) < common
    return pos, neg.reshape(-1, 3)


def assert_edges(pos, neg, k):
    """what the issue asks of a batch of 32 positives or more"""
    n = len(pos)
    g = neg.reshape(n, k, 3)
    ents = np.concatenate([pos[:, 0], pos[:, 2]])
    assert np.bincount(ents).max() >= 10                                                         # a hub entity
    assert (pos[:, 0] == pos[:, 2]).any()                                                        # h == t
    assert (g[:, :, 1] != pos[:, None, 1]).any()                                                 # another relation
    assert (g == pos[:, None, :]).all(2).any()                                                   # identical to its positive
    assert ((g[:, :, 0] == pos[:, None, 2]) & (pos[:, None, 0] != pos[:, None, 2])).any()        # head is the positive's tail
    rows = np.stack([pos[:, 0], pos[:, 2]], 1)
    apart = (g[:, :, 1] != pos[:, None, 1])
    for side in (0, 2):
        apart &= (g[:, :, side, None] != rows[:, None, :]).all(2)
    assert apart.any()                                                                           # shares no row


def hole_hinges(ent, rel, pos, neg, margin, k):
    """the hinge arguments l = margin + score(pos) - mean score(neg) of hole_loss per positive (float64), from hole_loss's own
    pieces; relu(l).sum() is checked against hole_loss itself"""
    e, r = sem._l2n(torch.tensor(ent)), sem._l2n(torch.tensor(rel))

    def score(tr):
        tr = sem._ids(tr)
        return -torch.sigmoid((sem._l2n(r[tr[:, 1]]) * sem.ccorr_fft(e[tr[:, 0]], e[tr[:, 2]])).sum(1))
    l = margin + score(pos) - score(neg).view(-1, k).mean(1)
    whole = float(sem.hole_loss(torch.tensor(ent), torch.tensor(rel), pos, neg, margin, k))
    assert abs(float(torch.relu(l).sum()) - whole) <= 1e-12 * max(abs(whole), 1.0)
    return l.numpy()


def _keep_first(ok, n, what):
    """the first n positives that pass `ok`; fewer than 1 % of those looked at may fail"""
    idx = np.flatnonzero(ok)[:n]
    assert len(idx) == n, what
    seen = idx[-1] + 1
    dropped = seen - n
    assert 100 * dropped < max(seen, 100), "%s: %d of %d positives lie on the kink" % (what, dropped, seen)
    return idx, int(dropped)


# ---- the restatements in both precisions -----------------------------------------------------------------------------------------
def _loss(model, vs, b):
    if model == "HolE":
        return sem.hole_loss(vs[0], vs[1], b["pos"], b["neg"], b["margin"], b["k"])
    if model == "SimplE":
        return sem.simple_loss(*vs, b["pos"], b["neg"])
    if model == "DistMult":
        return distmult_loss(vs[0], vs[1], b["pos"], b["neg"])
    if model == "JAPE":
        return jape_triple_loss(vs[0], vs[1], b["pos"], b["neg"], b["neg_alpha"])
    return weighted_pair_loss(vs[0], vs[1], b)[0]


def grads64(model, tables, b):
    """-> loss, [gradients]: the suite's float64 restatement of each step"""
    if model in ("HolE", "SimplE"):
        return sem.semantic_grads(model, tables, b["pos"], b["neg"], b["margin"], b["k"])
    if model == "DistMult":
        return distmult_grads(tables[0], tables[1], b["pos"], b["neg"])
    if model == "JAPE":
        return jape_triple_grads(tables[0], tables[1], b["pos"], b["neg"], b["neg_alpha"])
    loss, grads, _ = pair_grads(weighted_pair_loss, tables[0], tables[1], b)
    return loss, grads


@contextlib.contextmanager
def _direct_correlation():
    """hole_loss with ccorr_direct in place of the FFT form (the kernel sums directly as well)"""
    fft = sem.ccorr_fft
    sem.ccorr_fft = sem.ccorr_direct
    try:
        yield
    finally:
        sem.ccorr_fft = fft


def grads32(model, tables, b):
    """the same loss code on float32 tensors -> loss, [gradients] (as float64 arrays of float32 values).  HolE: the direct
    circular correlation, whose index tensor is n d^2 floats.  Up to 2^28 of them it is one run; above (d = 128 past the cap)
    the loss, a sum over positives, is taken in slices of 2^28 / (d^2 (k + 1)) positives (2.5 GB at the peak) whose gradients
    are added in float32, as one run would add them.  (Slices of 2,048 added in double made the proxy of the hub relation's row
    several times quieter than any fp32 sum of its 4,000 contributions: at d = 6, n = 16,389 the step then measured 0.36 and
    1.005 of the tolerance in two runs of the same case, the order of its atomics being free.)"""
    vs = [torch.tensor(np.asarray(v, np.float32), requires_grad=True) for v in tables]
    if model != "HolE":
        loss = _loss(model, vs, b)
        return float(loss.detach()), [g.numpy().astype(np.float64) for g in torch.autograd.grad(loss, vs, allow_unused=False)]
    n, k, loss, grads = len(b["pos"]), b["k"], 0.0, [np.zeros(v.shape, np.float32) for v in tables]
    step = max(1, 2 ** 28 // (tables[0].shape[1] ** 2 * (k + 1)))
    with _direct_correlation():
        for lo in range(0, n, step):
            part = dict(b, pos=b["pos"][lo:lo + step], neg=b["neg"][lo * k:(lo + step) * k])
            l = _loss(model, vs, part)
            for acc, g in zip(grads, torch.autograd.grad(l, vs)):
                acc += g.numpy()
            loss += float(l.detach())
    return loss, [g.astype(np.float64) for g in grads]


def abs_terms(model, tables, b, loss64):
    """sum |term| over the per-triple terms of the float64 loss.  HolE, SimplE, DistMult and the weighted pairs add terms that
    are never negative, so the sum is the loss; JAPE's negatives enter with -neg_alpha, its absolute sum is the loss at
    +neg_alpha."""
    if model != "JAPE":
        return abs(loss64)
    vs = [torch.tensor(t) for t in tables]
    return float(jape_triple_loss(vs[0], vs[1], b["pos"], b["neg"], -b["neg_alpha"]))


# ---- problems --------------------------------------------------------------------------------------------------------------------
def _tables(model, rng, dim):
    if model == "SimplE":
        return [_xavier(rng, N_ENT, dim), _xavier(rng, N_ENT, dim), _xavier(rng, N_REL, dim), _xavier(rng, N_REL, dim)]
    return [_xavier(rng, N_ENT, dim), _xavier(rng, N_REL, dim)]


@functools.lru_cache(maxsize=None)
def problem(model, dim, n_pos, k, margin=0.2, identical=False):
    """tables (float32-representable), a batch of exactly n_pos positives, the float64 loss and gradients, the float32 run.
    HolE and the weighted pairs have a hinge that may flip between fp32 and fp64 when its argument is near zero: positives whose
    float64 argument lies within 4 (d + 16) 2^-24 (HolE; 1e-5 for the pairs, as test_iptranse_gpu.py) of zero are left out here,
    with their negatives, before either side runs, and the batch is filled up from further draws.
    identical: every negative is its positive (HolE at margin 0: every hinge argument is 0.0 exactly)."""
    assert model in MODELS and (model != "WPair" or k == 1)
    rng = np.random.RandomState(1000 * dim + 7 * n_pos + k + 100000 * MODELS.index(model) + int(margin * 10))
    tables = _tables(model, rng, dim)
    spare = 0 if identical or model not in ("HolE", "WPair") else max(8, n_pos // 50)
    pos, neg = edge_batch(rng, n_pos + spare, k)
    b = dict(k=k, margin=PAIR_MARGIN if model == "WPair" else margin, neg_alpha=NEG_ALPHA)
    dropped = 0
    if identical:
        neg = np.repeat(pos, k, axis=0)
    elif model == "HolE":
        l = hole_hinges(tables[0], tables[1], pos, neg, margin, k)
        idx, dropped = _keep_first(np.abs(l) >= 4 * (dim + 16) * U24, n_pos, "HolE d=%d n=%d k=%d" % (dim, n_pos, k))
        pos, neg = pos[idx], neg.reshape(-1, k, 3)[idx].reshape(-1, 3)
        b["active"] = float((l[idx] > 0).mean())
        if margin == 0.0:
            assert 0.25 <= b["active"] <= 0.75, b["active"]
        if margin >= 1.0:
            assert b["active"] == 1.0                                    # the sigmoids lie in (0, 1)
    elif model == "WPair":
        w = rng.randint(1, 129, len(pos)) / 128.0                        # exact in fp32
        arg = weighted_pair_loss(torch.tensor(tables[0]), torch.tensor(tables[1]), dict(pos=pos, neg=neg, weight=w, margin=PAIR_MARGIN))[1]
        idx, dropped = _keep_first(np.abs(arg.numpy()) >= PAIR_KINK, n_pos, "WPair d=%d n=%d" % (dim, n_pos))
        pos, neg, b["weight"] = pos[idx], neg[idx], w[idx]
        b["active"] = float((arg.numpy()[idx] > 0).mean())
    assert len(pos) == n_pos and len(neg) == n_pos * k
    if n_pos >= 32 and not identical:
        assert_edges(pos, neg, k)
    b.update(pos=pos, neg=neg, dropped=dropped)
    loss64, g64 = grads64(model, tables, b)
    loss32, g32 = grads32(model, tables, b)
    return dict(model=model, dim=dim, tables=tables, batch=b, loss64=loss64, g64=g64, loss32=loss32, g32=g32,
                abs_terms=abs_terms(model, tables, b, loss64))


# ---- MTransE's mapping step ------------------------------------------------------------------------------------------------------
def mapping_grads(ent, M, links, alpha, dt=np.float64):
    """the SGD restatement of test_mapping_step_matches_oracle, its lines in the number type dt -> loss, d / d ent, d / d M"""
    d = M.shape[0]
    v, Mm = ent.astype(dt), M.astype(dt)
    inv = (1.0 / np.sqrt(np.maximum((v ** 2).sum(1, keepdims=True), dt(1e-12)))).astype(dt)
    y = v * inv
    e1, e2 = y[links[:, 0]], y[links[:, 1]]
    diff = e2 - e1 @ Mm
    orth = Mm @ Mm.T - np.eye(d, dtype=dt)
    alpha = dt(alpha)
    loss = alpha * ((diff ** 2).sum() + (orth ** 2).sum())
    gy = np.zeros_like(v)
    np.add.at(gy, links[:, 0], -2 * alpha * diff @ Mm.T)
    np.add.at(gy, links[:, 1], 2 * alpha * diff)
    gv = (gy - y * (y * gy).sum(1, keepdims=True)) * inv
    if dt == np.float64:
        ed = e1.T @ diff
    else:                                   # link by link, the order of mapping_update_kernel (see mapping_problem)
        ed = np.zeros((d, d), dt)
        for i in range(len(links)):
            ed += np.outer(e1[i], diff[i])
    gM = alpha * (dt(-2.0) * ed + dt(4.0) * orth @ Mm)
    terms = alpha * ((diff.astype(np.float64) ** 2).sum() + (orth.astype(np.float64) ** 2).sum())
    return float(loss), gv.astype(np.float64), gM.astype(np.float64), float(terms)


@functools.lru_cache(maxsize=None)
def mapping_problem(d, n, n_ent=900):
    """n links over the first n_ent - 100 entities, entities repeated on both sides (more links than entities, or two rows set
    equal), M near orthogonal as in test_mapping_step_matches_oracle.

    E32 of M.  numpy's float32 matmul sums E1^T Diff in blocks, and over 16,387 links its rounding is a fraction of that of any
    fixed left-to-right order; mapping_update_kernel keeps such an order on purpose (replicas get the same bits).  Against the
    matmul the step measured 1.57 (d = 100, n = 4,099) and 3.40 (d = 130, n = 16,387) times 4 E32 + recovery on M.  So the float32
    run of the restatement adds the n outer products link by link, the kernel's order; everything else is the same line."""
    rng = np.random.RandomState(d + n)
    ent = f32(rng.standard_normal((n_ent, d)))
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    M = f32(q + 0.05 * rng.standard_normal((d, d)))
    links = rng.randint(0, n_ent - 100, (n, 2)).astype(np.int32)
    if n >= 8:
        links[3, 0] = links[5, 0]
        links[4, 1] = links[6, 1]
        links[7, 1] = links[7, 0]
        assert len(np.unique(links[:, 0])) < n and len(np.unique(links[:, 1])) < n
    alpha = 5.0
    loss64, ge, gM, terms = mapping_grads(ent, M, links, alpha)
    loss32, ge32, gM32, _ = mapping_grads(ent, M, links, alpha, np.float32)
    return dict(ent=ent, M=M, links=links, alpha=alpha, loss64=loss64, g64=[ge, gM], loss32=loss32, g32=[ge32, gM32], abs_terms=terms)


# ---- IPTransE's path half --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def path_problem(n_rel, dim, n):
    """n path pairs with relations drawn evenly from the first n_rel - 4, so that A^T is written up to its last rows; no float64
    hinge argument within 1e-5 of zero (as the pairs above).  The reference is iptranse_loss with no triples: its path half."""
    from test_iptranse_cpu import iptranse_loss, path_hinge_arguments
    rng = np.random.RandomState(n_rel + dim)
    ent, rel = _xavier(rng, 50, dim), _xavier(rng, n_rel, dim)
    m = n + max(8, n // 50)
    q = rng.randint(0, n_rel - REL_TAIL, (m, 4)).astype(np.int32)
    w = rng.randint(1, 101, m).astype(np.float64)
    none = np.zeros((0, 3), np.int32)
    b = dict(paths=q[:, :3], neg_rel=q[:, 3], weight=w, margin=PAIR_MARGIN, path_parm=0.1, pos=none, neg=none)
    arg = path_hinge_arguments(sem._l2n(torch.tensor(rel)), b).numpy()
    idx, dropped = _keep_first(np.abs(arg) >= PAIR_KINK, n, "paths R=%d" % n_rel)
    b.update(paths=q[idx, :3], neg_rel=q[idx, 3], weight=w[idx], dropped=dropped, active=float((arg[idx] > 0).mean()))
    loss64, g64, _ = pair_grads(iptranse_loss, ent, rel, b)
    vs = [torch.tensor(np.asarray(v, np.float32), requires_grad=True) for v in (ent, rel)]
    l32 = iptranse_loss(vs[0], vs[1], b)[0]
    g32 = torch.autograd.grad(l32, vs[1])[0].numpy().astype(np.float64)
    return dict(tables=[ent, rel], dim=dim, batch=b, loss64=loss64, g64=g64[1], loss32=float(l32.detach()), g32=g32, abs_terms=abs(loss64))


# ---- the two checks --------------------------------------------------------------------------------------------------------------
TERM_BOUND = {"HolE": 0.5, "SimplE": 1.0, "DistMult": 1.0, "JAPE": 6.0, "WPair": 6.0}


def one_column_floor(p, i):
    """d = 1: what replaces E32 alone for table i of a problem, per row.

    A one-column row normalises to +-1 whatever it holds, so the exact gradient of every normalised table is zero and the step
    forms it as g_y - y (y . g_y) with y^2 = 1 + eta: what is left is eta g_y / |a|.  E32 then measures only how exactly torch's
    1 / sqrt happens to cancel (for SimplE, where the term inside cancels a second time, 1.8e-12 against the step's 7.4e-10 on a
    row of 1e-3), not the step's arithmetic.  A priori: y = a rsqrtf(a a) carries the rounding of a a (2^-25 after the root), the
    one ulp of rsqrtf (2^-23) and the product's rounding (2^-24), |y^2 - 1| < 2^-21; the dot product, the product and the
    difference of the projection round three more times at the size of g_y: together below 2^-20 |g_y| / |a|.  |g_y| is at most
    the number m of triples that name the row times the largest gradient one triple sends to a unit row: |ds| <= 1/4 on products
    of unit scalars, twice for the relation's two normalisations (HolE); |g| <= 1/2 on at most two unit factors (SimplE);
    sigmoid / N (DistMult); 2 c |h + r - t| <= 6 (JAPE, and the pairs with weight <= 1).  -> 2^-20 B m / |a| per row."""
    t0 = p["tables"][i]
    assert t0.shape[1] == 1
    b = p["batch"]
    cols = [1] if t0.shape[0] == N_REL else [0, 2]
    ids = np.concatenate([b["pos"][:, cols].reshape(-1), b["neg"][:, cols].reshape(-1)])
    m = np.bincount(ids, minlength=t0.shape[0])
    return 2.0 ** -20 * TERM_BOUND[p["model"]] * m / np.maximum(np.abs(t0[:, 0]), 1e-6)


def gradient_check(what, before, after, g64, g32, floor=0.0):
    """before, after: float32 [n, d] of one table around an SGD step with lr = 1.0 (see the module docstring)
    -> max row deviation / (4 E32), printed with the largest deviation / tolerance over the rows, which is what is asserted:
    every row against 4 E32 + 2^-24 |after row| (+ floor: one_column_floor at d = 1, else nothing).  The first ratio may pass 1
    where the gradient is so small that the rounding of `after` is most of what is measured (DistMult's mean over N triples)."""
    assert before.dtype == np.float32 and after.dtype == np.float32
    got = before.astype(np.float64) - after.astype(np.float64)
    dev = np.linalg.norm(got - g64, axis=1)
    e32 = float(np.linalg.norm(g32 - g64, axis=1).max())
    tol = 4 * e32 + U24 * np.linalg.norm(after.astype(np.float64), axis=1) + floor
    worst = int(np.argmax(dev / tol))
    ratio = float(dev.max() / (4 * e32)) if e32 > 0 else (0.0 if dev.max() == 0 else np.inf)
    print("%s: max row deviation %.3g, E32 %.3g, deviation / (4 E32) = %.3f; largest gradient row %.3g; deviation / tolerance "
          "at most %.3f (row %d: %.3g against %.3g)" % (what, dev.max(), e32, ratio, np.linalg.norm(g64, axis=1).max(),
                                                        dev[worst] / tol[worst], worst, dev[worst], tol[worst]))
    assert (dev <= tol).all(), "%s: row %d off by %.3g > %.3g" % (what, worst, dev[worst], tol[worst])
    return ratio


def loss_check(what, loss, p, dim):
    """|loss - loss64| <= (d + 32) 2^-24 sum |term|; prints measured / bound for the step and for the float32 restatement"""
    bound = (dim + 32) * U24 * p["abs_terms"]
    off, off32 = abs(loss - p["loss64"]), abs(p["loss32"] - p["loss64"])
    print("%s: loss %.12g (float64 %.12g), measured / bound = %.3f (float32 restatement %.3f)"
          % (what, loss, p["loss64"], off / bound if bound else off, off32 / bound if bound else off32))
    assert off <= bound, "%s: loss off by %.3g > %.3g" % (what, off, bound)
    return off / bound if bound else 0.0
