"""Float64 numpy restatements of MultiKE's graphs (reference approaches/multi_ke.py): the attribute CNN (`conv`, :154-176) with
analytic gradients, the row-wise terms of the other views, and the SGD steps built from them.  Everything runs on the CPU.

Assumptions about TF 1.x that nothing on this machine can pin (beyond A1-A10 of tests/test_tf1_golden.py):
  M1  tf.layers.conv2d(padding='same') with an even kernel pads AFTER: a [2, 4] kernel pads the rows (0, 1) and the columns (1, 2);
      the operation is a cross-correlation (no kernel flip), channels last.
  M2  tf.layers.batch_normalization(x, 2): the positional 2 is `axis`; training defaults to False, so the moving mean / variance
      keep their initial 0 / 1 and the layer is x gamma / sqrt(1 + 1e-3) + beta with gamma, beta of the axis' size, both trained.
  M3  tf.nn.l2_normalize(x, axis) = x rsqrt(max(sum x^2, 1e-12)); without an axis the sum runs over the whole tensor.
  M4  tf.layers.dense flattens nothing: `_flat` is the C-order reshape of [B, 2, d, 2], i.e. (row, column, channel)."""
import numpy as np

BN_C = 1.0 / np.sqrt(1.0 + 1e-3)
VARS = ("gamma", "beta", "K1", "b1", "K2", "b2", "W", "bd")


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def cnn_params(rng, d):
    """one parameter set at float32-representable values.  gamma near 1, beta small (TF starts them at 1 / 0: a trained state is
    what the gradients are checked at), glorot-sized kernels and dense weights"""
    return dict(gamma=f32(1.0 + 0.1 * rng.standard_normal(d)), beta=f32(0.1 * rng.standard_normal(d)),
                K1=f32(rng.uniform(-0.7, 0.7, (2, 4, 1, 2))), b1=f32(0.1 * rng.standard_normal(2)),
                K2=f32(rng.uniform(-0.5, 0.5, (2, 4, 2, 2))), b2=f32(0.1 * rng.standard_normal(2)),
                W=f32(rng.uniform(-1, 1, (4 * d, d)) * np.sqrt(6.0 / (5 * d))), bd=f32(0.1 * rng.standard_normal(d)))


def conv_same(x, K):
    """x [B, 2, d, ci], K [2, 4, ci, co] -> [B, 2, d, co]  (M1)"""
    B, _, d, ci = x.shape
    xp = np.zeros((B, 3, d + 3, ci), x.dtype)
    xp[:, :2, 1:d + 1] = x
    out = np.zeros((B, 2, d, K.shape[3]), x.dtype)
    for kh in range(2):
        for kw in range(4):
            out += xp[:, kh:kh + 2, kw:kw + d] @ K[kh, kw]
    return out


def conv_same_bwd(x, K, dout):
    B, _, d, ci = x.shape
    xp = np.zeros((B, 3, d + 3, ci), x.dtype)
    xp[:, :2, 1:d + 1] = x
    dxp, dK = np.zeros_like(xp), np.zeros_like(K)
    for kh in range(2):
        for kw in range(4):
            dK[kh, kw] = np.einsum('bijc,bijo->co', xp[:, kh:kh + 2, kw:kw + d], dout)
            dxp[:, kh:kh + 2, kw:kw + d] += dout @ K[kh, kw].T
    return dxp[:, :2, 1:d + 1], dK


def _l2n_rows(t, on=True):
    inv = 1.0 / np.sqrt(np.maximum((t ** 2).sum(1, keepdims=True), 1e-12)) if on else np.ones((len(t), 1), t.dtype)
    return t * inv, inv


def cnn_forward(p, ent, attr, lit, batch, weight=None, factor=1.0, l2n=True):
    """-> loss, cache.  weight: per-positive weights [B] or None."""
    a, v = attr[batch[:, 1]], lit[batch[:, 2]]
    u, inv = _l2n_rows(ent, l2n)
    h = u[batch[:, 0]]
    av = np.stack([a, v], 1)
    x = (av * p["gamma"] * BN_C + p["beta"])[..., None]
    z1 = np.tanh(conv_same(x, p["K1"]) + p["b1"])
    z2 = np.tanh(conv_same(z1, p["K2"]) + p["b2"])
    raw = np.sqrt((z2 ** 2).sum(2, keepdims=True))
    nr = np.maximum(raw, 1e-6)
    n = z2 / nr
    flat = n.reshape(len(batch), -1)
    t = np.tanh(flat @ p["W"] + p["bd"])
    tn = np.sqrt((t ** 2).sum())
    T = max(tn, 1e-6)
    y = t / T
    diff = h - y
    dist = (diff ** 2).sum(1)
    w = np.ones(len(batch)) if weight is None else np.asarray(weight, np.float64)
    terms = factor * w * np.logaddexp(0.0, dist)
    return float(terms.sum()), dict(av=av, u=u, inv=inv, x=x, z1=z1, z2=z2, raw=raw, nr=nr, n=n, flat=flat, t=t, tn=tn, T=T, y=y,
                                    diff=diff, dist=dist, w=w, terms=terms)


def cnn_loss_grads(p, ent, attr, lit, batch, weight=None, factor=1.0, l2n=True):
    """-> loss, parameter gradients (dict over VARS), d / d ent (the RAW table, through the row normalisation), d / d attr,
    d / d (normalised entity rows), cache"""
    loss, c = cnn_forward(p, ent, attr, lit, batch, weight, factor, l2n)
    s = factor * c["w"] / (1.0 + np.exp(-c["dist"]))
    gh = 2.0 * s[:, None] * c["diff"]
    g = -gh
    if c["tn"] >= 1e-6:
        dt = (g - c["y"] * (g * c["y"]).sum()) / c["T"]
    else:
        dt = g / c["T"]
    dpre = dt * (1.0 - c["t"] ** 2)
    grads = dict(bd=dpre.sum(0), W=c["flat"].T @ dpre)
    dn = (dpre @ p["W"].T).reshape(c["n"].shape)
    proj = np.where(c["raw"] >= 1e-6, (dn * c["n"]).sum(2, keepdims=True), 0.0)
    dz2 = (dn - c["n"] * proj) / c["nr"]
    dp2 = dz2 * (1.0 - c["z2"] ** 2)
    grads["b2"] = dp2.sum((0, 1, 2))
    dz1, grads["K2"] = conv_same_bwd(c["z1"], p["K2"], dp2)
    dp1 = dz1 * (1.0 - c["z1"] ** 2)
    grads["b1"] = dp1.sum((0, 1, 2))
    dx, grads["K1"] = conv_same_bwd(c["x"], p["K1"], dp1)
    dx = dx[..., 0]
    grads["gamma"] = (dx * c["av"] * BN_C).sum((0, 1))
    grads["beta"] = dx.sum((0, 1))
    g_attr = np.zeros_like(attr)
    np.add.at(g_attr, batch[:, 1], dx[:, 0] * p["gamma"] * BN_C)
    gy = np.zeros_like(ent)
    np.add.at(gy, batch[:, 0], gh)
    g_ent = (gy - c["u"] * (c["u"] * gy).sum(1, keepdims=True)) * c["inv"] if l2n else gy
    return loss, grads, g_ent, g_attr, gy, c


def through_l2n(table, gy, on=True):
    """the gradient w.r.t. the raw rows from the one w.r.t. the normalised rows"""
    if not on:
        return gy
    u, inv = _l2n_rows(table)
    return (gy - u * (u * gy).sum(1, keepdims=True)) * inv


# ---- the row-wise terms --------------------------------------------------------------------------------------------------------
def cross_term(A, B, rel, triples, coef=1.0, l2n=(True, True, True)):
    """coef sum |A[h] + rel[r] - B[t]|^2 on the normalised rows -> loss, gy_A, gy_B, gy_rel (w.r.t. the normalised rows)"""
    ua, ub, ur = _l2n_rows(A, l2n[0])[0], _l2n_rows(B, l2n[1])[0], _l2n_rows(rel, l2n[2])[0]
    x = ua[triples[:, 0]] + ur[triples[:, 1]] - ub[triples[:, 2]]
    ga, gb, gr = np.zeros_like(A), np.zeros_like(B), np.zeros_like(rel)
    np.add.at(ga, triples[:, 0], 2 * coef * x)
    np.add.at(gb, triples[:, 2], -2 * coef * x)
    np.add.at(gr, triples[:, 1], 2 * coef * x)
    return float(coef * (x ** 2).sum()), ga, gb, gr


def logistic_term(ent, rel, pos, neg, l2n=(True, True)):
    """losses.py:59-73 with the L2 score: sum softplus(|h + r - t|^2) over pos + sum softplus(-|h + r - t|^2) over neg
    -> loss, gy_ent, gy_rel (w.r.t. the normalised rows)"""
    u, ur = _l2n_rows(ent, l2n[0])[0], _l2n_rows(rel, l2n[1])[0]
    ge, gr, loss = np.zeros_like(ent), np.zeros_like(rel), 0.0
    for tr, sign in ((pos, 1.0), (neg, -1.0)):
        x = u[tr[:, 0]] + ur[tr[:, 1]] - u[tr[:, 2]]
        dist = (x ** 2).sum(1)
        loss += float(np.logaddexp(0.0, sign * dist).sum())
        c = (2 * sign / (1 + np.exp(-sign * dist)))[:, None] * x
        np.add.at(ge, tr[:, 0], c)
        np.add.at(ge, tr[:, 2], -c)
        np.add.at(gr, tr[:, 1], c)
    return loss, ge, gr


def wsoft_term(A, B, rel, triples, rel_weight, coef=1.0, l2n=(True, True, True), triple_weight=None):
    """coef sum w[r] softplus(|A[h] + rel[r] - B[t]|^2)   (positive_loss_with_weight, multi_ke.py:294-300); triple_weight: the
    weights per triple, as the reference feeds them, in place of rel_weight[r]"""
    ua, ub, ur = _l2n_rows(A, l2n[0])[0], _l2n_rows(B, l2n[1])[0], _l2n_rows(rel, l2n[2])[0]
    x = ua[triples[:, 0]] + ur[triples[:, 1]] - ub[triples[:, 2]]
    dist = (x ** 2).sum(1)
    w = coef * (np.asarray(rel_weight, A.dtype)[triples[:, 1]] if triple_weight is None else np.asarray(triple_weight, A.dtype))
    c = (2 * w / (1 + np.exp(-dist)))[:, None] * x
    ga, gb, gr = np.zeros_like(A), np.zeros_like(B), np.zeros_like(rel)
    np.add.at(ga, triples[:, 0], c)
    np.add.at(gb, triples[:, 2], -c)
    np.add.at(gr, triples[:, 1], c)
    return float((w * np.logaddexp(0.0, dist)).sum()), ga, gb, gr


def pull_term(A, B, ids, coef=1.0, l2n=(True, True)):
    """coef sum |A[e] - B[e]|^2 over ids (an id that repeats counts as often) -> loss, gy_A, gy_B"""
    ua, ub = _l2n_rows(A, l2n[0])[0], _l2n_rows(B, l2n[1])[0]
    x = ua[ids] - ub[ids]
    ga, gb = np.zeros_like(A), np.zeros_like(B)
    np.add.at(ga, ids, 2 * coef * x)
    np.add.at(gb, ids, -2 * coef * x)
    return float(coef * (x ** 2).sum()), ga, gb


# ---- problems ------------------------------------------------------------------------------------------------------------------
def cnn_problem(seed, B, d, n_ent=50, n_attr=7, n_lit=40, nets=2):
    """tables, parameter sets and a batch with a repeated entity, a repeated attribute and literal; net 0 is weighted"""
    rng = np.random.RandomState(seed)
    ents = [f32(rng.standard_normal((n_ent, d)) / np.sqrt(d)) for _ in range(nets)]
    attr = f32(rng.uniform(-1, 1, (n_attr, d)) * np.sqrt(6.0 / (n_attr + d)))
    lit = rng.standard_normal((n_lit, d))
    lit = f32(lit / np.linalg.norm(lit, axis=1, keepdims=True))
    batch = np.stack([rng.randint(0, n_ent - 5, B), rng.randint(0, n_attr - 1, B), rng.randint(0, n_lit, B)], 1).astype(np.int32)
    if B >= 3:
        batch[2, 0] = batch[0, 0]
        batch[1, 1] = batch[0, 1]
        batch[2, 2] = batch[1, 2]
    aw = f32(rng.randint(1, 65, n_attr) / 64.0)
    params = [cnn_params(rng, d) for _ in range(nets)]
    return dict(ents=ents, attr=attr, lit=lit, batch=batch, aw=aw, params=params, d=d, factors=[1.0, 1.0][:nets])


def cnn_problem_grads(P):
    """-> total loss, per net (grads, g_ent, gy), the summed attribute gradient, caches"""
    loss, per, g_attr, caches = 0.0, [], np.zeros_like(P["attr"]), []
    for k, (p, ent) in enumerate(zip(P["params"], P["ents"])):
        w = P["aw"][P["batch"][:, 1]] if k == 0 else None
        l, g, ge, ga, gy, c = cnn_loss_grads(p, ent, P["attr"], P["lit"], P["batch"], w, P["factors"][k])
        loss += l
        per.append((g, ge, gy))
        g_attr += ga
        caches.append(c)
    return loss, per, g_attr, caches


def cnn_sgd_step(P, lr):
    """one SGD step of the two-net attribute step in place -> loss"""
    loss, per, g_attr, _ = cnn_problem_grads(P)
    for k, (g, ge, _) in enumerate(per):
        for name in VARS:
            P["params"][k][name] = P["params"][k][name] - lr * g[name]
        P["ents"][k] = P["ents"][k] - lr * ge
    P["attr"] = P["attr"] - lr * g_attr
    return loss
