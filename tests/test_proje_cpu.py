"""ProjE (models/neural/proje.py of the reference) restated in numpy: the log-uniform candidate sampler, the forward pass, the
gradients and TF's dense Adam.  The restatement is held to the reference's own graph (tests/golden/proje_graph.npz: loss in
float64, gradients by central finite differences) and is what the device tests compare oea_proje_step with.

The TF ops the reference calls are not part of it and no fixture pins them; what is ASSUMED of them (documented TF-1 behaviour):
  A1  tf.nn.log_uniform_candidate_sampler(unique=True): P(c) = (log(c + 2) - log(c + 1)) / log(E + 1); draws one after another
      until S distinct classes have appeared; num_tries = the number of draws; expected count Q(c) = -expm1(num_tries log1p(-P(c))).
  A2  tf.nn.nce_loss(num_true=1, remove_accidental_hits=False, subtract_log_q=True): logits = x . w + b - log Q, labels 1 for the
      true column and 0 for the sampled ones, sigmoid cross entropy max(x, 0) - x z + log1p(exp(-|x|)) summed over the columns;
      the candidates are shared by the batch; no gradient into them or into Q.
  A3  tf.contrib.layers.batch_norm defaults: is_training=True (batch statistics, biased variance), decay irrelevant, center=True,
      scale=False, epsilon=1e-3; reuse=True shares beta.
  A4  tf.train.AdamOptimizer: beta1 0.9, beta2 0.999, epsilon 1e-8, lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t), dense in effect
      for IndexedSlices too (m and v decay everywhere), duplicate rows summed first.
  A5  get_variable without an initializer: glorot_uniform; on a 1-D shape fan_in = fan_out = the length.
"""
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "proje_graph.npz")
CASES = ("proje_d5", "proje_d16")
VARS = ("ent_embeds", "rel_embeds", "entity_w", "entity_b", "input_bn_beta", "mlp_w", "mlp_bias", "output_bn_beta")
SAMPLER_TAG = 0x50726a45
BN_EPS = 1e-3


# ---- Philox4x32-10 (csrc/common.h) ---------------------------------------------------------------------------------------
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """vectorised over c0 (uint32 array); the other counter words and the key are scalars -> uint32 [n, 4]"""
    M0, M1, W0, W1, mask = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF
    c0 = np.asarray(c0, np.uint64)
    c1, c2, c3 = (np.full_like(c0, v, dtype=np.uint64) for v in (c1, c2, c3))
    k0, k1 = int(k0), int(k1)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & np.uint64(mask), p1 >> np.uint64(32), p1 & np.uint64(mask)
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + W0) & mask, (k1 + W1) & mask
    return np.stack([c0, c1, c2, c3], 1).astype(np.uint32)


def sampler_words(seed, step, n):
    """the first n 32-bit words of the draw sequence of (seed, step): try t = word t & 3 of the Philox block t >> 2"""
    blocks = (n + 3) // 4
    w = philox4x32_10(np.arange(blocks, dtype=np.uint64), SAMPLER_TAG, step & 0xFFFFFFFF, (step >> 32) & 0xFFFFFFFF,
                      seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return w.reshape(-1)[:n]


def thresholds(n_classes):
    return np.log(np.arange(2, n_classes + 2, dtype=np.float64)) / np.log(np.float64(n_classes + 1))


def classes_of(words, table):
    """the first c with u < T[c], u = (w + 0.5) 2^-32"""
    u = (words.astype(np.float64) + 0.5) * 2.0 ** -32
    return np.searchsorted(table, u, side="right")


def log_q(classes, num_tries, n_classes):
    c = np.asarray(classes, np.float64)
    p = (np.log(c + 2.0) - np.log(c + 1.0)) / np.log(np.float64(n_classes + 1))
    return np.log(-np.expm1(num_tries * np.log1p(-p)))


def log_uniform_reference(n_classes, n_sampled, seed, step):
    """A1 -> (ids [S] in the order of first appearance, num_tries, log Q of the ids in fp64)"""
    table = thresholds(n_classes)
    n = 4 * n_sampled
    while True:
        cls = classes_of(sampler_words(seed, step, n), table)
        uniq, first = np.unique(cls, return_index=True)
        if len(uniq) >= n_sampled:
            first = np.sort(first)[:n_sampled]
            num_tries = int(first[-1]) + 1
            ids = cls[first]
            return ids.astype(np.int64), num_tries, log_q(ids, num_tries, n_classes)
        assert n < 64 * n_sampled, "more than 64 S tries"
        n = min(4 * n, 64 * n_sampled)


# ---- the model -----------------------------------------------------------------------------------------------------------
def _bn(x, beta, dt):
    mean = x.mean(0, dtype=dt)
    var = ((x - mean) ** 2).mean(0, dtype=dt)
    istd = (1.0 / np.sqrt(var + dt(BN_EPS))).astype(dt)
    xh = (x - mean) * istd
    return xh + beta, xh, istd


def _bn_back(dy, xh, istd):
    return istd * (dy - dy.mean(0) - xh * (dy * xh).mean(0))


def _l2n(x, dt):
    inv = (1.0 / np.sqrt(np.maximum((x * x).sum(1, keepdims=True, dtype=dt), dt(1e-12)))).astype(dt)
    return x * inv, inv


ZERO_GRADS = (4, 6)     # input_bn_beta, mlp_bias


def proje_loss_and_grads(variables, pos, sampled, num_tries, dt=np.float64, with_scale=False):
    """loss (dt) and the dense gradients of the eight variables (order VARS).

    The gradients of the input beta and of mlp_bias are ZERO identically: both shift every row of `out` by the same vector, and
    the output batch norm subtracts the column mean (sum_b dout = 0).  What any implementation computes for them is the
    cancellation noise of a sum over the batch, so a bound relative to max|ref| says nothing there.  with_scale=True also returns
    {index: scale}: the sum over the batch of the magnitudes of the terms that cancel (per column, the largest column) -- the
    quantity that rounding noise of these two sums is proportional to."""
    ent, rel, W, bvec, beta_in, mlp_w, mlp_b, beta_out = [np.asarray(v, dt) for v in variables]
    n_ent = ent.shape[0]
    h, r, t = (np.asarray(pos)[:, i].astype(np.int64) for i in range(3))
    sampled = np.asarray(sampled, np.int64)
    en, einv = _l2n(ent[h], dt)
    rn, rinv = _l2n(rel[r], dt)
    a, ah, ais = _bn(en, beta_in, dt)
    c, ch, cis = _bn(rn, beta_in, dt)
    z = (a + c)
    out = z * mlp_w + mlp_b
    x, oh, ois = _bn(out, beta_out, dt)
    lq_t = log_q(t, num_tries, n_ent).astype(dt)
    lq_s = log_q(sampled, num_tries, n_ent).astype(dt)
    true = (x * W[t]).sum(1, dtype=dt) + bvec[t] - lq_t
    samp = x @ W[sampled].T + bvec[sampled] - lq_s
    xent = lambda v, y: np.maximum(v, 0) - v * y + np.log1p(np.exp(-np.abs(v)))        # noqa: E731
    loss = xent(true, 1.0).sum(dtype=dt) + xent(samp, 0.0).sum(dtype=dt)
    sig = lambda v: (1.0 / (1.0 + np.exp(-v))).astype(dt)                                 # noqa: E731
    dtrue, dsamp = sig(true) - dt(1.0), sig(samp)
    dx = dtrue[:, None] * W[t] + dsamp @ W[sampled]
    gW, gb = np.zeros_like(W), np.zeros_like(bvec)
    np.add.at(gW, t, dtrue[:, None] * x)
    np.add.at(gb, t, dtrue)
    np.add.at(gW, sampled, dsamp.T @ x)
    np.add.at(gb, sampled, dsamp.sum(0, dtype=dt))
    g_beta_out = dx.sum(0, dtype=dt)
    dout = _bn_back(dx, oh, ois)
    g_bias = dout.sum(0, dtype=dt)
    g_w = (dout * z).sum(0, dtype=dt)
    dz = dout * mlp_w
    g_beta_in = 2 * dz.sum(0, dtype=dt)
    den, drn = _bn_back(dz, ah, ais), _bn_back(dz, ch, cis)
    g_ent, g_rel = np.zeros_like(ent), np.zeros_like(rel)
    np.add.at(g_ent, h, (den - en * (en * den).sum(1, keepdims=True, dtype=dt)) * einv)
    np.add.at(g_rel, r, (drn - rn * (rn * drn).sum(1, keepdims=True, dtype=dt)) * rinv)
    grads = [g_ent, g_rel, gW, gb, g_beta_in, g_w, g_bias, g_beta_out]
    if not with_scale:
        return loss, grads
    cols = (ois * (np.abs(dx) + np.abs(dx.mean(0)) + np.abs(oh) * np.abs((dx * oh).mean(0)))).sum(0)
    return loss, grads, {4: float((2 * np.abs(mlp_w) * cols).max()), 6: float(cols.max())}


def adam_dense(p, g, m, v, lr, t, dt=np.float64):
    """A4, in place"""
    lr_t = dt(lr * np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t))
    m[...] = dt(0.9) * m + dt(1.0 - 0.9) * g
    v[...] = dt(0.999) * v + dt(1.0 - 0.999) * g * g
    p[...] = p - lr_t * m / (np.sqrt(v) + dt(1e-8))


def proje_reference_step(variables, moments_m, moments_v, pos, sampled, num_tries, t, lr, dt=np.float64):
    """one step in place on lists of arrays of dtype dt; sampled / num_tries as the sampler gave them -> the batch loss"""
    loss, grads = proje_loss_and_grads(variables, pos, sampled, num_tries, dt)
    for p, g, m, v in zip(variables, grads, moments_m, moments_v):
        adam_dense(p, g.astype(dt), m, v, lr, t, dt)
    return float(loss)


def make_variables(rng, n_ent, n_rel, dim):
    """the eight variables as the model initialises them (xavier tables, glorot vectors), with betas moved off zero so that
    every term of the graph is exercised; float32-representable float64"""
    from openea_amd.modules.base.initializers import glorot_uniform_host, xavier_host
    v = [xavier_host(rng, (n_ent, dim)), xavier_host(rng, (n_rel, dim)), xavier_host(rng, (n_ent, dim)), xavier_host(rng, (n_ent,)),
         0.1 * glorot_uniform_host(rng, (dim,)), glorot_uniform_host(rng, (dim,)), glorot_uniform_host(rng, (dim,)),
         0.1 * glorot_uniform_host(rng, (dim,))]
    return [np.asarray(x, np.float32).astype(np.float64) for x in v]


def zipf_batch(rng, n_ent, n_rel, n, sampled):
    """n positives: heads under a Zipf(1.1) law over [0, n_ent - 50) with ONE head in the first 20 rows, relations from
    [0, n_rel - 2), the last 10 labels equal, the first 5 labels taken from `sampled`; the last 50 entities and 2 relations appear
    nowhere (sampled ids may lie there: the caller leaves them out where it checks untouched rows).  A batch shorter than 40 rows
    repeats its head in (n + 1) // 2 rows and its label in n // 2 rows only: when EVERY row has the same head, the input batch
    norm sees a constant column and the gradient of that entity row is zero identically (its terms cancel over the batch), which
    a bound relative to max|ref| cannot test."""
    used = n_ent - 50
    p = 1.0 / np.arange(1, used + 1) ** 1.1
    pos = np.stack([rng.choice(used, n, p=p / p.sum()), rng.randint(0, n_rel - 2, n), rng.randint(0, used, n)], 1).astype(np.int32)
    pos[:min(20, (n + 1) // 2), 0] = pos[0, 0]
    pos[n - min(10, n // 2):, 2] = pos[-1, 2]
    inside = [s for s in sampled if s < used][:min(5, n // 2)]
    pos[:len(inside), 2] = inside
    return pos


def fixture_case(z, case):
    variables = [z["%s_var_%s" % (case, n)] for n in VARS]
    return variables, z[case + "_pos"], z[case + "_sampled"], int(z[case + "_num_tries"][0])


# ---- tests ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_reference_graph(case):
    z = np.load(GOLDEN)
    variables, pos, sampled, num_tries = fixture_case(z, case)
    loss, grads, scale = proje_loss_and_grads(variables, pos, sampled, num_tries, with_scale=True)
    ref = float(z[case + "_loss"][0])
    assert abs(loss - ref) <= 1e-9 * abs(ref)
    for i, (name, g) in enumerate(zip(VARS, grads)):
        want = z["%s_grad_%s" % (case, name)]
        if i in ZERO_GRADS:
            # identically zero (see proje_loss_and_grads): the fixture's central difference (eps = 1e-6) of a float64 loss holds
            # a few ulps of the loss over 2 eps, the restatement a few float64 roundings of the terms that cancel
            assert np.abs(want).max() <= 8 * np.spacing(ref) / 2e-6, name
            assert np.abs(g).max() <= 1e-12 * scale[i], name
            continue
        assert np.abs(g - want).max() <= 1e-5 * np.abs(want).max(), name


@pytest.mark.parametrize("case", CASES)
def test_fixture_batches_hold_the_hard_rows(case):
    z = np.load(GOLDEN)
    _, pos, sampled, _ = fixture_case(z, case)
    assert len(set(pos[:, 0])) < len(pos) and len(set(pos[:, 2])) < len(pos)
    assert set(pos[:, 2]) & set(sampled) and (pos[:, 0] == pos[:, 2]).sum() == 1
    assert len(set(sampled)) == len(sampled)


SAMPLER_SHAPES = [(300, 64), (97, 97), (1000, 257)]


@pytest.mark.parametrize("n_classes,n_sampled", SAMPLER_SHAPES)
def test_sampler_restatement(n_classes, n_sampled):
    for seed, step in ((11, 0), (2 ** 40 + 5, 3)):
        ids, num_tries, lq = log_uniform_reference(n_classes, n_sampled, seed, step)
        assert len(ids) == n_sampled == len(set(ids)) and ids.min() >= 0 and ids.max() < n_classes
        # a plain sequential loop over the same draws
        table = thresholds(n_classes)
        words = sampler_words(seed, step, 64 * n_sampled)
        seen, order, tries = set(), [], 0
        for w in words:
            tries += 1
            c = int(classes_of(np.array([w]), table)[0])
            if c not in seen:
                seen.add(c)
                order.append(c)
                if len(order) == n_sampled:
                    break
        assert order == list(ids) and tries == num_tries
        c = ids.astype(np.float64)
        p = (np.log(c + 2) - np.log(c + 1)) / np.log(n_classes + 1.0)
        np.testing.assert_allclose(np.exp(lq), -np.expm1(num_tries * np.log1p(-p)), rtol=1e-12)
        assert (np.exp(lq) > 0).all() and (np.exp(lq) <= 1).all()


@pytest.mark.parametrize("n_classes,n_sampled", SAMPLER_SHAPES)
def test_table_search_equals_the_exp_form(n_classes, n_sampled):
    table = thresholds(n_classes)
    assert table[-1] == 1.0
    words = sampler_words(1234 + n_classes, 7, 10 ** 6)
    u = (words.astype(np.float64) + 0.5) * 2.0 ** -32
    direct = np.floor(np.exp(u * np.log(n_classes + 1.0))).astype(np.int64) - 1
    assert np.array_equal(classes_of(words, table), direct)


def test_philox_matches_the_oracle():
    from oracle import cport
    got = philox4x32_10(np.array([0, 1, 77]), 2, 3, 4, 5, 6)
    for row, c0 in zip(got, (0, 1, 77)):
        assert np.array_equal(row, cport.philox([c0, 2, 3, 4], [5, 6]))


# ---- class protocol --------------------------------------------------------------------------------------------------------
def _model(**over):
    from openea_amd.models.neural import ProjE
    from openea_amd.run.default_args import get_args
    m = ProjE()
    m.set_args(get_args("ProjE", output="/tmp/oea_proje_cpu/", training_data="synthetic/tiny/", dataset_division="f/", **over))
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


def test_dim_above_the_kernel_limit_is_refused_before_any_table():
    import types
    m = _model(dim=132)
    m.kgs = types.SimpleNamespace(entities_num=40, relations_num=5)
    with pytest.raises(NotImplementedError):
        m.init()
    assert m.ent_embeds is None


@pytest.mark.parametrize("scale", ["15K", "100K"])
def test_default_args_match_the_shipped_files(scale):
    import json
    from openea_amd.run.default_args import get_args
    shipped = json.load(open(os.path.join(HERE, "golden", "proje_args_%s.json" % scale)))
    ours = get_args("ProjE", scale).__dict__
    for k, v in shipped.items():
        assert k in ours and ours[k] == v, (k, v, ours.get(k))
    assert set(ours) == set(shipped)
