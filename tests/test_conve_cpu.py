"""ConvE (models/neural/conve.py of the reference) restated in numpy: the dropout masks, the forward pass, the analytic gradients
of the fourteen variables and TF's dense Adam.  The restatement is held to the reference's own graph
(tests/golden/conve_graph.npz: loss in float64, gradients by central finite differences) and is what the device tests compare
oea_conve_step with.  The sampler and Philox come from test_proje_cpu.py.

What is ASSUMED of TensorFlow continues A1-A5 of test_proje_cpu.py, which all still apply (documented TF-1 behaviour; no fixture
pins it):
  A6  tf.layers.batch_normalization without training= runs in inference mode on the initial moving statistics: mean 0, variance
      1, epsilon 1e-3, never updated; each of the three BNs is y = x gamma / sqrt(1 + 1e-3) + beta; gamma starts at ones, beta at
      zeros, both trainable; the default axis is -1 (the y columns for BN1, the d columns for BN3), BN2 uses axis=1 (the filters).
      (The reading tests/golden/tf_shim.py:371-387 uses for AliNet.)
  A7  tf.layers.conv2d(padding='same', data_format='channels_first', use_bias=True): the kernel variable is [3, 3, 1, F],
      glorot-uniform with fans 9 and 9 F, the bias starts at zeros; zero padding; a cross-correlation (no kernel flip).
  A8  tf.contrib.layers.fully_connected(ocnn, d): activation relu; weights xavier_initializer (uniform, fans 2 d F and d), biases
      zeros.
  A9  tf.nn.dropout(v, keep_prob) = v / keep_prob * mask, on in every training step (the graph has no training flag); the
      reference's random stream cannot be reproduced, the mask is this project's (include/openea_hip.h, restated in mask_lanes).
  A10 nothing else of the graph is new: nce_loss, the sampler, Adam and the row normalisation are as in ProjE.
"""
import os

import numpy as np
import pytest

from test_proje_cpu import _l2n, adam_dense, log_q, philox4x32_10

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "conve_graph.npz")
CASES = ("conve_d6", "conve_d16")
VARS = ("ent_embeds", "rel_embeds", "entity_w", "entity_b", "gamma1", "beta1", "kern", "cbias", "gamma2", "beta2", "fcW", "fcb",
        "gamma3", "beta3")
MASK_TAG = 0x436f6e00
BN_EPS = 1e-3


def dim_factorization(d):
    import math
    half = int(math.sqrt(d)) + 1
    while d % half > 0:
        half -= 1
    return half, d // half


# ---- the masks -------------------------------------------------------------------------------------------------------------
def mask_threshold(keep_prob):
    """an element is kept iff its 16-bit lane < floor(keep_prob 65536), keep_prob as the float32 the device is given"""
    return int(np.floor(np.float64(np.float32(keep_prob)) * 65536.0))


def mask_lanes(seed, step, layer, row, n):
    """the 16-bit lanes of elements 0 .. n - 1 of (layer, batch row) at `step`: lane e & 7 of Philox(counter = (e >> 3, tag | layer,
    row, step mod 2^32), key = seed); lane l = the low (l even) or high (l odd) half of word l >> 1"""
    w = philox4x32_10(np.arange((n + 7) // 8, dtype=np.uint64), MASK_TAG | layer, row, step & 0xFFFFFFFF, seed & 0xFFFFFFFF,
                      (seed >> 32) & 0xFFFFFFFF)
    return np.stack([w & np.uint32(0xFFFF), w >> np.uint32(16)], 2).reshape(-1)[:n]


def dropout_masks(seed, step, n_rows, dim, filters, keep_prob):
    """(m0 [B, 2 d], m1 [B, 2 d F]) as 0 / 1 float64; keep_prob 1 draws nothing"""
    n0, n1 = 2 * dim, 2 * dim * filters
    if keep_prob >= 1:
        return np.ones((n_rows, n0)), np.ones((n_rows, n1))
    thr = mask_threshold(keep_prob)
    m0 = np.stack([mask_lanes(seed, step, 0, b, n0) < thr for b in range(n_rows)])
    m1 = np.stack([mask_lanes(seed, step, 1, b, n1) < thr for b in range(n_rows)])
    return m0.astype(np.float64), m1.astype(np.float64)


# ---- the model -------------------------------------------------------------------------------------------------------------
def _taps(sp, n_rows, n_cols):
    """the nine shifted views of a padded image batch [B, 2x + 2, y + 2], in the order (0,0) (0,1) ... (2,2)"""
    return [sp[:, di:di + n_rows, dj:dj + n_cols] for di in range(3) for dj in range(3)]


def conve_loss_and_grads(variables, pos, sampled, num_tries, m0, m1, keep_prob, dt=np.float64, with_margin=False):
    """loss (dt) and the dense gradients of the fourteen variables (order VARS; kern as [3, 3, 1, F]).  with_margin=True also
    returns the smallest |z| / sum |terms of z| over the two relu pre-activations (z1 gamma2 c + beta2 and z2)."""
    ent, rel, W, bvec, g1, b1, kern, cb, g2, b2, fcw, fcb, g3, b3 = [np.asarray(v, dt) for v in variables]
    n_ent, d = ent.shape
    F = cb.shape[0]
    kern = kern.reshape(3, 3, 1, F)
    x, y = dim_factorization(d)
    B = len(pos)
    c = dt(1.0 / np.sqrt(1.0 + BN_EPS))
    keep = dt(keep_prob)
    m0 = np.asarray(m0, dt).reshape(B, 2 * x, y)
    m1 = np.asarray(m1, dt).reshape(B, F, 2 * x, y)
    h, r, t = (np.asarray(pos)[:, i].astype(np.int64) for i in range(3))
    sampled = np.asarray(sampled, np.int64)
    en, einv = _l2n(ent[h], dt)
    rn, rinv = _l2n(rel[r], dt)
    img = np.concatenate([en.reshape(B, x, y), rn.reshape(B, x, y)], 1)
    s = (img * (g1 * c) + b1) / keep * m0
    sp = np.pad(s, ((0, 0), (1, 1), (1, 1)))
    taps = _taps(sp, 2 * x, y)
    kw = kern.reshape(9, F)
    z1 = sum(tp[:, None] * kw[i][None, :, None, None] for i, tp in enumerate(taps)) + cb[None, :, None, None]
    g2c = (g2 * c)[None, :, None, None]
    u = z1 * g2c + b2[None, :, None, None]
    a = np.maximum(u, 0) / keep * m1
    af = a.reshape(B, -1)
    z2 = af @ fcw + fcb
    X = np.maximum(z2, 0) * (g3 * c) + b3
    lq_t = log_q(t, num_tries, n_ent).astype(dt)
    lq_s = log_q(sampled, num_tries, n_ent).astype(dt)
    true = (X * W[t]).sum(1, dtype=dt) + bvec[t] - lq_t
    samp = X @ W[sampled].T + bvec[sampled] - lq_s
    xent = lambda v, z: np.maximum(v, 0) - v * z + np.log1p(np.exp(-np.abs(v)))        # noqa: E731
    loss = xent(true, 1.0).sum(dtype=dt) + xent(samp, 0.0).sum(dtype=dt)
    sig = lambda v: (1.0 / (1.0 + np.exp(-v))).astype(dt)                                 # noqa: E731
    dtrue, dsamp = sig(true) - dt(1.0), sig(samp)
    dX = dtrue[:, None] * W[t] + dsamp @ W[sampled]
    gW, gb = np.zeros_like(W), np.zeros_like(bvec)
    np.add.at(gW, t, dtrue[:, None] * X)
    np.add.at(gb, t, dtrue)
    np.add.at(gW, sampled, dsamp.T @ X)
    np.add.at(gb, sampled, dsamp.sum(0, dtype=dt))
    g_b3 = dX.sum(0, dtype=dt)
    g_g3 = (dX * np.maximum(z2, 0) * c).sum(0, dtype=dt)
    dz2 = dX * (g3 * c) * (z2 > 0)
    g_fcb = dz2.sum(0, dtype=dt)
    g_fcw = af.T @ dz2
    da = (dz2 @ fcw.T).reshape(B, F, 2 * x, y)
    du = da / keep * m1 * (u > 0)
    g_g2 = (du * z1 * c).sum((0, 2, 3), dtype=dt)
    g_b2 = du.sum((0, 2, 3), dtype=dt)
    dz1 = du * g2c
    g_cb = dz1.sum((0, 2, 3), dtype=dt)
    g_kern = np.stack([(dz1 * tp[:, None]).sum((0, 2, 3), dtype=dt) for tp in taps]).reshape(3, 3, 1, F)
    dsp = np.zeros_like(sp)
    i = 0
    for di in range(3):
        for dj in range(3):
            dsp[:, di:di + 2 * x, dj:dj + y] += (dz1 * kw[i][None, :, None, None]).sum(1, dtype=dt)
            i += 1
    dv = dsp[:, 1:-1, 1:-1] / keep * m0
    g_g1 = (dv * img * c).sum((0, 1), dtype=dt)
    g_b1 = dv.sum((0, 1), dtype=dt)
    dimg = dv * (g1 * c)
    den, drn = dimg[:, :x].reshape(B, d), dimg[:, x:].reshape(B, d)
    g_ent, g_rel = np.zeros_like(ent), np.zeros_like(rel)
    np.add.at(g_ent, h, (den - en * (en * den).sum(1, keepdims=True, dtype=dt)) * einv)
    np.add.at(g_rel, r, (drn - rn * (rn * drn).sum(1, keepdims=True, dtype=dt)) * rinv)
    grads = [g_ent, g_rel, gW, gb, g_g1, g_b1, g_kern, g_cb, g_g2, g_b2, g_fcw, g_fcb, g_g3, g_b3]
    if not with_margin:
        return loss, grads
    mag1 = (sum(np.abs(tp[:, None] * kw[i][None, :, None, None]) for i, tp in enumerate(taps)) + np.abs(cb)[None, :, None, None]) \
        * np.abs(g2c) + np.abs(b2)[None, :, None, None]
    mag2 = np.abs(af) @ np.abs(fcw) + np.abs(fcb)
    live = (m1 > 0)                 # a masked element's sign decides nothing
    margin = min(float((np.abs(u) / mag1)[live].min()) if live.any() else np.inf, float((np.abs(z2) / mag2).min()))
    return loss, grads, margin


def conve_reference_step(variables, moments_m, moments_v, pos, sampled, num_tries, m0, m1, keep_prob, t, lr, dt=np.float64):
    """one step in place on lists of arrays of dtype dt -> the batch loss"""
    loss, grads = conve_loss_and_grads(variables, pos, sampled, num_tries, m0, m1, keep_prob, dt)
    for p, g, m, v in zip(variables, grads, moments_m, moments_v):
        adam_dense(p, g.astype(dt).reshape(p.shape), m, v, lr, t, dt)
    return float(loss)


def make_variables(rng, n_ent, n_rel, dim, filters):
    """the fourteen variables as the model initialises them (A6-A8), with the gammas, betas and biases moved off ones / zeros so
    that every term of the graph is exercised; float32-representable float64"""
    from openea_amd.modules.base.initializers import xavier_host
    y = dim_factorization(dim)[1]
    K = 2 * dim * filters
    uni = lambda shape, fi, fo: rng.uniform(-np.sqrt(6.0 / (fi + fo)), np.sqrt(6.0 / (fi + fo)), shape)     # noqa: E731
    near = lambda n, mid: mid + 0.2 * rng.uniform(-1, 1, n)                                                   # noqa: E731
    v = [xavier_host(rng, (n_ent, dim)), xavier_host(rng, (n_rel, dim)), xavier_host(rng, (n_ent, dim)), xavier_host(rng, (n_ent,)),
         near(y, 1.0), near(y, 0.0), uni((3, 3, 1, filters), 9, 9 * filters), near(filters, 0.0), near(filters, 1.0),
         near(filters, 0.0), uni((K, dim), K, dim), near(dim, 0.0), near(dim, 1.0), near(dim, 0.0)]
    return [np.asarray(x, np.float32).astype(np.float64) for x in v]


def fixture_case(z, case):
    variables = [z["%s_var_%s" % (case, n)] for n in VARS]
    return variables, z[case + "_pos"], z[case + "_sampled"], int(z[case + "_num_tries"][0]), z[case + "_m0"], z[case + "_m1"], \
        float(z[case + "_keep_prob"][0])


# ---- tests -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_reference_graph(case):
    z = np.load(GOLDEN)
    variables, pos, sampled, num_tries, m0, m1, keep = fixture_case(z, case)
    loss, grads = conve_loss_and_grads(variables, pos, sampled, num_tries, m0, m1, keep)
    ref = float(z[case + "_loss"][0])
    assert abs(loss - ref) <= 1e-12 * abs(ref)
    for name, g in zip(VARS, grads):
        want = z["%s_grad_%s" % (case, name)]
        assert np.abs(g.reshape(want.shape) - want).max() <= 1e-6 * np.abs(want).max(), name


@pytest.mark.parametrize("case", CASES)
def test_fixture_batches_hold_the_hard_rows(case):
    z = np.load(GOLDEN)
    _, pos, sampled, _, m0, m1, keep = fixture_case(z, case)
    assert len(set(pos[:, 0])) < len(pos) and len(set(pos[:, 2])) < len(pos)
    assert set(pos[:, 2]) & set(sampled) and (pos[:, 0] == pos[:, 2]).sum() == 1
    assert len(set(sampled)) == len(sampled)
    assert keep == 0.7 and 0 < m0.mean() < 1 and 0 < m1.mean() < 1
    n_ent, n_rel, d, n_s, F, seed, step = (int(v) for v in z[case + "_shape"])
    w0, w1 = dropout_masks(seed, step, len(pos), d, F, keep)
    assert np.array_equal(w0, m0) and np.array_equal(w1, m1)


def test_dim_factorization():
    from openea_amd import ops
    want = {5: (1, 5), 6: (3, 2), 7: (1, 7), 8: (2, 4), 16: (4, 4), 75: (5, 15), 97: (1, 97), 100: (10, 10), 128: (8, 16)}
    for d, xy in want.items():
        assert ops.dim_factorization(d) == xy and dim_factorization(d) == xy


def test_masks_do_not_depend_on_the_batch_size():
    a0, a1 = dropout_masks(9, 4, 3, 10, 3, 0.7)
    b0, b1 = dropout_masks(9, 4, 7, 10, 3, 0.7)
    assert np.array_equal(a0, b0[:3]) and np.array_equal(a1, b1[:3])
    assert not np.array_equal(b1[0], b1[1])
    # a shorter row is a prefix of a longer one: the element index alone selects the lane
    assert np.array_equal(mask_lanes(9, 4, 1, 2, 50), mask_lanes(9, 4, 1, 2, 500)[:50])


def test_masks_differ_between_steps_and_layers():
    base = mask_lanes(9, 4, 0, 2, 4096)
    assert not np.array_equal(base, mask_lanes(9, 5, 0, 2, 4096))
    assert not np.array_equal(base, mask_lanes(9, 4, 1, 2, 4096))
    assert not np.array_equal(base, mask_lanes(10, 4, 0, 2, 4096))
    assert np.array_equal(base, mask_lanes(9, 4 + 2 ** 32, 0, 2, 4096))        # the counter holds the step mod 2^32


def test_kept_share():
    assert mask_threshold(0.7) == 45875
    lanes = mask_lanes(12345, 6, 1, 3, 10 ** 6)
    assert lanes.max() < 65536
    share = (lanes < mask_threshold(0.7)).mean()
    assert abs(share - 45875 / 65536) <= 0.002, share
    m0, m1 = dropout_masks(1, 0, 2, 6, 3, 1.0)
    assert m0.all() and m1.all()


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_gradients_come_in_the_dtype_asked_for(dt):
    rng = np.random.RandomState(3)
    variables = make_variables(rng, 30, 4, 6, 2)
    pos = np.array([[0, 1, 2], [3, 1, 4], [0, 0, 2]])
    sampled = np.array([5, 9, 2, 11])
    m0, m1 = dropout_masks(3, 0, 3, 6, 2, 0.7)
    loss, grads = conve_loss_and_grads(variables, pos, sampled, 7, m0, m1, 0.7, dt)
    assert loss.dtype == dt and all(g.dtype == dt for g in grads)
    ref_loss, ref = conve_loss_and_grads(variables, pos, sampled, 7, m0, m1, 0.7)
    assert abs(float(loss) - float(ref_loss)) <= 1e-5 * abs(float(ref_loss))


# ---- class protocol --------------------------------------------------------------------------------------------------------
def _model(**over):
    from openea_amd.models.neural import ConvE
    from openea_amd.run.default_args import get_args
    m = ConvE()
    m.set_args(get_args("ConvE", output="/tmp/oea_conve_cpu/", training_data="synthetic/tiny/", dataset_division="f/", **over))
    return m


@pytest.mark.parametrize("over", [dict(optimizer="Adagrad"), dict(init="normal"), dict(alignment_module="swapping"),
                                  dict(eval_metric="euclidean"), dict(ent_l2_norm=False), dict(rel_l2_norm=False),
                                  dict(dnn_neg_nums=1), dict(dnn_neg_nums=0)])
def test_init_asserts(over):
    import types
    m = _model(**over)
    m.kgs = types.SimpleNamespace(entities_num=40, relations_num=5)
    with pytest.raises(AssertionError):
        m.check_args()


@pytest.mark.parametrize("over", [dict(dim=132), dict(filter_num=65), dict(filter_num=0)])
def test_shapes_above_the_kernel_limits_are_refused_before_any_table(over):
    import types
    m = _model(**over)
    m.kgs = types.SimpleNamespace(entities_num=40, relations_num=5)
    with pytest.raises(NotImplementedError):
        m.init()
    assert m.ent_embeds is None


def test_class_is_found_like_proje(capsys):
    from openea_amd.models import neural
    from openea_amd.models.neural import ProjE
    m = neural.ConvE()
    assert isinstance(m, ProjE) and m.kernel_size == (3, 3)
    assert "kernel_size (3, 3)" in capsys.readouterr().out


@pytest.mark.parametrize("scale", ["15K", "100K"])
def test_default_args_match_the_shipped_files(scale):
    import json
    from openea_amd.run.default_args import get_args
    shipped = json.load(open(os.path.join(HERE, "golden", "conve_args_%s.json" % scale)))
    ours = get_args("ConvE", scale).__dict__
    for k, v in shipped.items():
        assert k in ours and ours[k] == v, (k, v, ours.get(k))
    assert set(ours) == set(shipped)
