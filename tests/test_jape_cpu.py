"""JAPE without a GPU: float64 restatements of its triple loss (approaches/jape.py:74-84 of the reference) and of its similarity
loss over a thresholded CSR (jape.py:86-98, 127-149), the numpy restatement of the keyed permutation behind
oea_sample_distinct (csrc/sample_distinct.hip), and the host functions of approaches/attr2vec.py.  The GPU tests
(test_jape_gpu.py) hold the device kernels to these."""
import os

import numpy as np
import pytest

from test_proje_cpu import log_q, log_uniform_reference, philox4x32_10

torch = pytest.importorskip("torch")

from openea_amd.approaches import attr2vec as a2v  # noqa: E402  (what this file is about: without it nothing here can run)
from openea_amd.approaches.jape import JAPE, JapeTrainer  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "jape_graph.npz")
ATTR_CASES = ("attr_d5", "attr_d16")
ATTR_VARS = ("embeds", "nce_weights", "nce_biases")
DISTINCT_TAG = 0x64697374
FD_TOL = 1e-6        # central differences at 1e-6 against analytic gradients: the tolerance test_proje_cpu.py uses


def _l2n(x):
    """tf.nn.l2_normalize(x, 1): x * rsqrt(max(sum x^2, 1e-12))"""
    return x * torch.rsqrt(torch.clamp((x * x).sum(1, keepdim=True), min=1e-12))


def _ids(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.long)


# ---- Attr2Vec ----------------------------------------------------------------------------------------------------------------
def _softplus(v):
    return np.maximum(v, 0) + np.log1p(np.exp(-np.abs(v)))


def _sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def _l2n_np(x, dt):
    inv = (1.0 / np.sqrt(np.maximum((x * x).sum(1, keepdims=True, dtype=dt), dt(1e-12)))).astype(dt)
    return x * inv, inv


def attr2vec_loss_and_grads(variables, pairs, sampled, num_tries, dt=np.float64):
    """attr2vec.py:113-123 with tf.nn.nce_loss written out (num_true = 1, accidental hits kept, log Q subtracted, sigmoid cross
    entropy summed over the true and the sampled columns, the mean over the batch) -> loss, [d / d embeds, d / d nce_weights,
    d / d nce_biases]; both tables enter through l2_normalize (xavier_init(..., True))"""
    emb, w, b = (np.asarray(v, dt) for v in variables)
    n_attr = emb.shape[0]
    pairs, sampled = np.asarray(pairs, np.int64), np.asarray(sampled, np.int64)
    xn, inv_x = _l2n_np(emb, dt)
    wn, inv_w = _l2n_np(w, dt)
    ins, lab = pairs[:, 0], pairs[:, 1]
    n = dt(len(pairs))
    x = xn[ins]
    true = (x * wn[lab]).sum(1) + b[lab] - log_q(lab, num_tries, n_attr).astype(dt)
    samp = x @ wn[sampled].T + (b[sampled] - log_q(sampled, num_tries, n_attr).astype(dt))
    loss = (_softplus(-true) + _softplus(samp).sum(1)).sum(dtype=dt) / n
    d_true, d_samp = -_sigmoid(-true) / n, _sigmoid(samp) / n
    gx, gw, gb = np.zeros_like(emb), np.zeros_like(w), np.zeros_like(b)
    np.add.at(gx, ins, d_true[:, None] * wn[lab] + d_samp @ wn[sampled])
    np.add.at(gw, lab, d_true[:, None] * x)
    np.add.at(gw, sampled, d_samp.T @ x)
    np.add.at(gb, lab, d_true)
    np.add.at(gb, sampled, d_samp.sum(0))
    back = lambda g, y, inv: inv * (g - y * (y * g).sum(1, keepdims=True))          # noqa: E731
    return float(loss), [back(gx, xn, inv_x), back(gw, wn, inv_w), gb]


def attr2vec_reference_step(variables, accs, pairs, sampled, num_tries, lr, dt=np.float64):
    """one Adagrad step in place (tf.train.AdagradOptimizer, accumulators from 0.1; a zero gradient changes nothing) -> batch mean"""
    loss, grads = attr2vec_loss_and_grads(variables, pairs, sampled, num_tries, dt)
    for v, a, g in zip(variables, accs, grads):
        a += g * g
        v -= dt(lr) * g / np.sqrt(a)
    return loss


def attr2vec_variables(rng, n_attr, dim):
    lim = np.sqrt(6.0 / (n_attr + dim))
    f32 = lambda a: a.astype(np.float32).astype(np.float64)                          # noqa: E731
    return [f32(rng.uniform(-lim, lim, (n_attr, dim))), f32(rng.uniform(-lim, lim, (n_attr, dim))), f32(rng.uniform(-0.2, 0.2, n_attr))]


def attr2vec_batch(rng, n_attr, n, sampled, absent):
    """n (input, label) pairs without `absent`: a repeated input, a repeated label, a label that is among the samples, input == label"""
    ok = np.array([a for a in range(n_attr) if a != absent])
    pairs = ok[rng.randint(0, len(ok), (n, 2))]
    pairs[: n // 4, 0] = pairs[0, 0]
    pairs[n // 4: n // 2, 1] = pairs[n // 4, 1]
    pairs[-1, 1] = [c for c in sampled if c != absent][0]
    pairs[-2, 1] = pairs[-2, 0]
    return pairs.astype(np.int32)


def test_attr2vec_restatement_gradient_is_the_derivative_of_its_loss():
    rng = np.random.RandomState(9)
    n_attr, dim, n_s = 14, 5, 4
    variables = attr2vec_variables(rng, n_attr, dim)
    sampled, num_tries, _ = log_uniform_reference(n_attr, n_s, 20190719, 0)
    pairs = attr2vec_batch(rng, n_attr, 6, sampled, 13)
    loss, grads = attr2vec_loss_and_grads(variables, pairs, sampled, num_tries)
    assert loss > 0 and all(np.abs(g).max() > 0 for g in grads)
    h = 1e-6
    for i, g in enumerate(grads):
        for idx in [tuple(t) for t in np.argwhere(np.abs(g) > 0)[::5]]:
            vs = [v.copy() for v in variables]
            vs[i][idx] += h
            up = attr2vec_loss_and_grads(vs, pairs, sampled, num_tries)[0]
            vs[i][idx] -= 2 * h
            dn = attr2vec_loss_and_grads(vs, pairs, sampled, num_tries)[0]
            assert abs((up - dn) / (2 * h) - g[idx]) <= 1e-7 * max(1.0, np.abs(g).max()), (i, idx)
    assert np.abs(grads[0][13]).max() == 0                      # attribute 13 is no pair's input


# ---- the triple loss ---------------------------------------------------------------------------------------------------------
def jape_triple_loss(ent, rel, pos, neg, neg_alpha, ent_l2_norm=True, rel_l2_norm=True):
    """jape.py:74-83 in float64: sum_pos |h + r - t|^2 - neg_alpha sum_neg |h + r - t|^2 (init_embeddings shows the tables
    through l2_normalize when the flags are set)"""
    e = _l2n(ent) if ent_l2_norm else ent
    w = _l2n(rel) if rel_l2_norm else rel

    def score(tr):
        tr = _ids(tr)
        x = e[tr[:, 0]] + w[tr[:, 1]] - e[tr[:, 2]]
        return (x * x).sum()
    return score(pos) - neg_alpha * score(neg)


def jape_triple_grads(ent, rel, pos, neg, neg_alpha, **kw):
    """-> loss, [d loss / d ent, d loss / d rel] (float64 numpy)"""
    vs = [torch.tensor(np.asarray(v, np.float64), requires_grad=True) for v in (ent, rel)]
    loss = jape_triple_loss(vs[0], vs[1], pos, neg, neg_alpha, **kw)
    return float(loss.detach()), [g.numpy() for g in torch.autograd.grad(loss, vs)]


def jape_reference_step(tables, accs, pos, neg, neg_alpha, lr, optimizer="Adagrad", **kw):
    """one step of (ent, rel) in place (float64); tf.train.AdagradOptimizer, accumulators from 0.1: a zero gradient leaves a row
    and its accumulator unchanged.  -> the batch sum"""
    loss, grads = jape_triple_grads(tables[0], tables[1], pos, neg, neg_alpha, **kw)
    for v, a, g in zip(tables, accs, grads):
        if optimizer == "Adagrad":
            a += g * g
            v -= lr * g / np.sqrt(a)
        else:
            v -= lr * g
    return loss


def jape_batch(rng, n_ent, n_rel, n, k, unused=20):
    """n positives over the first n_ent - unused entities: one entity in many triples, triples with h == t; k corruptions of
    head or tail per positive (each shares two rows with its positive), a few of them with another relation"""
    used = n_ent - unused
    pos = np.stack([rng.randint(0, used, n), rng.randint(0, n_rel - 1, n), rng.randint(0, used, n)], 1).astype(np.int32)
    pos[: n // 4, 0] = pos[0, 0]
    pos[n // 4: n // 4 + 4, 2] = pos[n // 4: n // 4 + 4, 0]
    neg = np.repeat(pos, k, axis=0)
    side = rng.randint(0, 2, n * k) * 2
    neg[np.arange(n * k), side] = rng.randint(0, used, n * k)
    neg[::7, 1] = rng.randint(0, n_rel - 1, len(neg[::7]))
    return pos, neg


# ---- the similarity loss -------------------------------------------------------------------------------------------------------
def l2n_rows(x):
    x = np.asarray(x, np.float64)
    return x / np.sqrt(np.maximum((x * x).sum(-1, keepdims=True), 1e-12))


def jape_sim_loss_reference(ent, ref1_ids, ref2_ids, indptr, col, val, rows, beta):
    """jape.py:91-95 with attr_sim_mat[idx, :] as CSR rows: beta sum_i |l2n(ent)[ref1[rows_i]] - l2n(sim[rows_i, :] @ l2n(ent)[ref2])|^2"""
    e = l2n_rows(ent)
    loss = 0.0
    for r in np.asarray(rows):
        lo, hi = int(indptr[r]), int(indptr[r + 1])
        t = (np.asarray(val[lo:hi], np.float64)[:, None] * e[np.asarray(ref2_ids)[col[lo:hi]]]).sum(0)
        d = e[ref1_ids[r]] - l2n_rows(t)
        loss += float((d * d).sum())
    return beta * loss


def sim_csr_reference(e1, e2, threshold):
    """sim_mat[sim_mat < threshold] = 0 (jape.py:148) as a CSR of the float64 products"""
    s = np.asarray(e1, np.float64) @ np.asarray(e2, np.float64).T
    keep = s >= threshold
    indptr = np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int64)
    return indptr, np.nonzero(keep)[1].astype(np.int32), s[keep], s


# ---- the keyed permutation -------------------------------------------------------------------------------------------------------
def _mix32(x):
    m = np.uint64(0xFFFFFFFF)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & m
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & m
    return x ^ (x >> np.uint64(16))


def sample_distinct_reference(n, m, seed, step):
    """csrc/sample_distinct.hip: the first m images of a 6-round Feistel network over max(2, ceil(log2 n)) bits, cycle-walked into
    [0, n); round keys = Philox4x32-10(counter = (step lo, step hi, tag, 0 | 1), key = (seed lo, seed hi)) -> int64 [m]"""
    bits = 2
    while (1 << bits) < n:
        bits += 1
    rbits = bits // 2
    lbits = bits - rbits
    lmask, rmask = np.uint64((1 << lbits) - 1), np.uint64((1 << rbits) - 1)
    c0 = np.array([step & 0xFFFFFFFF], np.uint64)
    ka, kb = ((seed & 0xFFFFFFFF), (seed >> 32) & 0xFFFFFFFF)
    wa = philox4x32_10(c0, (step >> 32) & 0xFFFFFFFF, DISTINCT_TAG, 0, ka, kb)[0]
    wb = philox4x32_10(c0, (step >> 32) & 0xFFFFFFFF, DISTINCT_TAG, 1, ka, kb)[0]
    key = [np.uint64(w) for w in (wa[0], wa[1], wa[2], wa[3], wb[0], wb[1])]
    x = np.arange(m, dtype=np.uint64)
    todo = np.ones(m, bool)
    while todo.any():
        v = x[todo]
        left, right = v >> np.uint64(rbits), v & rmask
        for q in range(0, 6, 2):
            left = (left ^ _mix32(right ^ key[q])) & lmask
            right = (right ^ _mix32(left ^ key[q + 1])) & rmask
        x[todo] = (left << np.uint64(rbits)) | right
        todo = x >= np.uint64(n)
    return x.astype(np.int64)


@pytest.mark.parametrize("n", [1, 2, 1000, 2 ** 20 + 3])
def test_permutation_restatement_is_a_bijection(n):
    for seed, step in ((20190719, 0), (2 ** 40 + 5, 2 ** 33 + 7)):
        full = sample_distinct_reference(n, n, seed, step)
        assert full.min() == 0 and full.max() == n - 1 and len(np.unique(full)) == n
        m = max(1, n // 3)
        assert np.array_equal(sample_distinct_reference(n, m, seed, step), full[:m])       # a prefix of the same permutation
    if n >= 1000:
        assert not np.array_equal(sample_distinct_reference(n, n, 1, 0), sample_distinct_reference(n, n, 1, 1))
        assert not np.array_equal(sample_distinct_reference(n, n, 1, 0), sample_distinct_reference(n, n, 2, 0))


def test_permutation_draws_are_uniform():
    """64 steps of m = 256 from n = 1000: element i is drawn c_i times, c_i ~ Binomial(64, p), p = m / n; chi^2 = sum (c_i - mu)^2 /
    (mu (1 - p)), mu = 64 p, has mean n (n - 1 degrees of freedom after the constraint sum c_i = 64 m) and variance 2 n.  numpy's
    own permutation sampling gives 999 +- 42 over 200 repetitions, so n +- 6 sqrt(2 n) is six standard deviations."""
    n, m, steps = 1000, 256, 64
    counts = np.zeros(n)
    for step in range(steps):
        counts += np.bincount(sample_distinct_reference(n, m, 20190719, step), minlength=n)
    p = m / n
    mu = steps * p
    chi2 = float(((counts - mu) ** 2).sum() / (mu * (1 - p)))
    print("chi^2 = %.1f (expected %d +- %.1f)" % (chi2, n, np.sqrt(2 * n)))
    assert abs(chi2 - n) <= 6 * np.sqrt(2 * n)


# ---- the restatements themselves ---------------------------------------------------------------------------------------------
def test_triple_loss_has_no_hinge_and_a_negative_weight():
    """the gradient of the restatement against central differences, and the two properties no OEA_LOSS_* kind has: the negatives
    enter with weight -neg_alpha and nothing is clipped (a loss below zero still has a gradient)"""
    rng = np.random.RandomState(3)
    ent, rel = rng.standard_normal((30, 6)) * 0.5, rng.standard_normal((5, 6)) * 0.5
    pos, neg = jape_batch(rng, 30, 5, 12, 2, unused=4)
    loss, (ge, gr) = jape_triple_grads(ent, rel, pos, neg, 0.1)
    only_pos, _ = jape_triple_grads(ent, rel, pos, neg, 0.0)
    only_neg, _ = jape_triple_grads(ent, rel, neg, pos[:0], 0.0)
    assert abs(loss - (only_pos - 0.1 * only_neg)) <= 1e-12 * abs(only_pos)
    big, (ge_big, _) = jape_triple_grads(ent, rel, pos, neg, 50.0)
    assert big < 0 and np.abs(ge_big).max() > 0
    h = 1e-6
    for tab, g, which in ((ent, ge, 0), (rel, gr, 1)):
        for idx in ((int(pos[0, 0]), 2), (1, 3)) if which == 0 else ((int(pos[0, 1]), 0),):
            tabs = [ent.copy(), rel.copy()]
            tabs[which][idx] += h
            up = float(jape_triple_loss(torch.tensor(tabs[0]), torch.tensor(tabs[1]), pos, neg, 0.1))
            tabs[which][idx] -= 2 * h
            dn = float(jape_triple_loss(torch.tensor(tabs[0]), torch.tensor(tabs[1]), pos, neg, 0.1))
            assert abs((up - dn) / (2 * h) - g[idx]) <= 1e-6 * max(1.0, np.abs(g).max())
    # h == t: the two entity halves cancel and only the relation moves
    _, (g1, g2) = jape_triple_grads(ent, rel, np.array([[2, 1, 2]]), np.array([[2, 1, 2]]), 0.0)
    assert np.abs(g1).max() <= 1e-15 and np.abs(g2[1]).max() > 0


def test_similarity_loss_restatement_equals_the_dense_form():
    """the CSR form against jape.py:91-95 written densely; an empty row gives l2n(0) = 0, so its term is |ref1 row|^2 = 1"""
    rng = np.random.RandomState(5)
    ent = rng.standard_normal((40, 7))
    ref1, ref2 = rng.permutation(40)[:9], rng.permutation(40)[:11]
    a, b = l2n_rows(rng.standard_normal((9, 4))), l2n_rows(rng.standard_normal((11, 4)))
    a[4] = 0.0
    indptr, col, val, dense = sim_csr_reference(a, b, 0.3)
    assert indptr[5] == indptr[4] and indptr[-1] == len(col) > 9
    rows = np.array([0, 4, 7, 7, 2])
    sim = np.where(dense >= 0.3, dense, 0.0)[rows]
    e = l2n_rows(ent)
    want = 0.01 * ((e[ref1[rows]] - l2n_rows(sim @ e[ref2])) ** 2).sum()
    got = jape_sim_loss_reference(ent, ref1, ref2, indptr, col, val, rows, 0.01)
    assert abs(got - want) <= 1e-12 * want
    only_empty = jape_sim_loss_reference(ent, ref1, ref2, indptr, col, val, np.array([4]), 1.0)
    assert abs(only_empty - 1.0) <= 1e-12


# ---- the reference's own graphs (tests/golden/jape_graph.npz, make_jape_golden.py) ---------------------------------------------
def attr_fixture_case(z, case):
    return ([z["%s_var_%s" % (case, n)] for n in ATTR_VARS], z[case + "_pairs"], z[case + "_sampled"], int(z[case + "_num_tries"][0]))


def sim_fixture_csr(z):
    """the fixture's dense 4 x 4 similarity block as the CSR the device holds"""
    sim = z["sim_d5_mat"]
    keep = sim != 0
    return np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int64), np.nonzero(keep)[1].astype(np.int32), sim[keep]


@pytest.mark.parametrize("case", ATTR_CASES)
def test_attr2vec_restatement_equals_reference_graph(case):
    z = np.load(GOLDEN)
    variables, pairs, sampled, num_tries = attr_fixture_case(z, case)
    n_attr, d, n_b, n_s = z[case + "_shape"]
    assert pairs.shape == (n_b, 2) and len(sampled) == n_s and variables[0].shape == (n_attr, d)
    assert len(set(pairs[:, 0])) < n_b and len(set(pairs[:, 1])) < n_b                          # a repeated input, a repeated label
    assert set(pairs[:, 1]) & set(sampled) and (pairs[:, 0] == pairs[:, 1]).any()
    for v in variables:
        assert np.array_equal(v, v.astype(np.float32).astype(np.float64))
    loss, grads = attr2vec_loss_and_grads(variables, pairs, sampled, num_tries)
    assert abs(loss - z[case + "_loss"][0]) <= 1e-9 * abs(z[case + "_loss"][0])
    for name, g in zip(ATTR_VARS, grads):
        ref = z["%s_grad_%s" % (case, name)]
        assert g.shape == ref.shape and np.abs(ref).max() > 0, name
        assert np.abs(g - ref).max() <= FD_TOL * max(1.0, np.abs(ref).max()), name


def test_triple_restatement_equals_reference_graph():
    z = np.load(GOLDEN)
    pos, neg = z["triple_d5_pos"], z["triple_d5_neg"]
    n_ent, n_rel, d, k = z["triple_d5_shape"]
    assert k == 2 and len(neg) == k * len(pos) and (pos[:, 0] == pos[:, 2]).any()
    assert any(set(neg[2 * p + j][[0, 2]]) & set(pos[p][[0, 2]]) for p in range(len(pos)) for j in range(2))
    loss, grads = jape_triple_grads(z["triple_d5_var_ent_embeds"], z["triple_d5_var_rel_embeds"], pos, neg,
                                    float(z["triple_d5_neg_alpha"][0]))
    assert abs(loss - z["triple_d5_loss"][0]) <= 1e-9 * abs(z["triple_d5_loss"][0])
    for name, g in zip(("ent_embeds", "rel_embeds"), grads):
        ref = z["triple_d5_grad_" + name]
        assert np.abs(ref).max() > 0 and np.abs(g - ref).max() <= FD_TOL * max(1.0, np.abs(ref).max()), name


def test_similarity_restatement_equals_reference_graph():
    z = np.load(GOLDEN)
    indptr, col, val = sim_fixture_csr(z)
    assert indptr[2] == indptr[1]                                                               # the empty row
    ent, beta = z["triple_d5_var_ent_embeds"], float(z["sim_d5_beta"][0])
    got = jape_sim_loss_reference(ent, z["sim_d5_ref1"], z["sim_d5_ref2"], indptr, col, val, z["sim_d5_idx"], beta)
    assert abs(got - z["sim_d5_loss"][0]) <= 1e-9 * z["sim_d5_loss"][0]
    empty = jape_sim_loss_reference(ent, z["sim_d5_ref1"], z["sim_d5_ref2"], indptr, col, val, np.array([1, 1, 1]), beta)
    assert abs(empty - z["sim_d5_empty_row_loss"][0]) <= 1e-9 * empty and abs(empty - 3 * beta) <= 1e-12


# ---- the host functions ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_kgs():
    from openea_amd.modules.load.synth import make_kgs
    return make_kgs("tiny", mode="sharing", seed=0, attributes=True)


def test_host_functions_equal_the_reference(tiny_kgs, capsys):
    z = np.load(GOLDEN)
    sel1, sel2, sel = a2v.get_kgs_popular_attributes(tiny_kgs, 0.9)
    assert "total selected attributes %d" % len(sel) in capsys.readouterr().out
    assert sorted(sel1) == z["host_selected1"].tolist() and sorted(sel2) == z["host_selected2"].tolist()
    assert sorted(sel) == z["host_selected"].tolist()
    data = a2v.generate_training_data(tiny_kgs, threshold=0.9)
    assert np.array_equal(np.asarray(data, np.int32).reshape(-1, 2), z["host_training_data"])           # order and orientation
    rowptr, cols, vals = a2v.entity_attribute_csr(tiny_kgs, sel)
    mean = np.zeros((tiny_kgs.entities_num, z["host_attr_embeds"].shape[1]))
    for i in range(tiny_kgs.entities_num):
        lo, hi = rowptr[i], rowptr[i + 1]
        mean[i] = (vals[lo:hi, None].astype(np.float64) * z["host_attr_embeds"][cols[lo:hi]]).sum(0)
    norm = np.linalg.norm(mean, axis=1, keepdims=True)
    np.testing.assert_allclose(mean / np.where(norm == 0, 1.0, norm), z["host_ent_mat"], rtol=0, atol=2e-6)
    # get_ent_embeds_from_attributes itself runs on the device: test_jape_gpu.py holds it to host_ent_mat / host_ent_mat_few
    few = a2v.entity_attribute_csr(tiny_kgs, set(z["host_selected_few"].tolist()))[0]
    assert np.array_equal(np.diff(few) == 0, np.abs(z["host_ent_mat_few"]).sum(1) == 0)                  # the same zero rows


def test_synthetic_attributes_keep_the_default_and_follow_the_survey(tiny_kgs):
    from openea_amd.modules.load import synth
    plain = synth.make_kgs("tiny", mode="sharing", seed=0)
    assert plain.attributes_num == 0 and plain.kg1.attribute_triples_num == 0
    assert plain.kg1.relation_triples_list == tiny_kgs.kg1.relation_triples_list and plain.train_links == tiny_kgs.train_links
    assert synth.ATTRIBUTES["EN-FR-15K-V1"] == ((308, 404), (73121, 67167))
    assert synth.ATTRIBUTES["EN-FR-100K-V1"] == ((466, 519), (497729, 426672))
    (a1, a2), (t1, t2) = synth.ATTRIBUTES["tiny"]
    assert tiny_kgs.kg1.attribute_triples_num == t1 and tiny_kgs.kg2.attribute_triples_num == t2
    assert tiny_kgs.kg1.attributes_num <= a1 and tiny_kgs.kg2.attributes_num <= a2 and 24 <= tiny_kgs.attributes_num <= a1 + a2
    # aligned entities share a latent profile: how much two entities' attribute sets overlap in KG1 predicts how much their
    # counterparts' sets overlap in KG2 (Jaccard against Jaccard over ~3000 random pairs), and not under a shuffled alignment
    att1, att2 = synth.generate_attribute_triples("tiny", 0)
    sets = []
    for att in (att1, att2):
        by_ent = [set() for _ in range(400)]
        for e, a, _ in att:
            by_ent[int(e.split("/e")[1])].add(a)
        sets.append(by_ent)
    rng = np.random.RandomState(0)
    ii, jj = rng.randint(0, 400, 3000), rng.randint(0, 400, 3000)
    ii, jj = ii[ii != jj], jj[ii != jj]
    jac = lambda s, i, j: len(s[i] & s[j]) / max(len(s[i] | s[j]), 1)                                   # noqa: E731
    j1 = np.array([jac(sets[0], i, j) for i, j in zip(ii, jj)])
    j2 = np.array([jac(sets[1], i, j) for i, j in zip(ii, jj)])
    perm = rng.permutation(400)
    j2_shuffled = np.array([jac(sets[1], perm[i], perm[j]) for i, j in zip(ii, jj)])
    corr, corr_shuffled = np.corrcoef(j1, j2)[0, 1], np.corrcoef(j1, j2_shuffled)[0, 1]
    print("Jaccard correlation across the alignment %.3f, shuffled %.3f" % (corr, corr_shuffled))
    sigma = 1.0 / np.sqrt(len(ii))                       # of a sample correlation when there is none
    assert corr > 6 * sigma and abs(corr_shuffled) < 6 * sigma


# ---- the classes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", ["15K", "100K"])
def test_default_args_match_the_shipped_files(scale):
    import json
    from openea_amd.run.default_args import get_args
    shipped = json.load(open(os.path.join(HERE, "golden", "jape_args_%s.json" % scale)))
    ours = get_args("JAPE", scale).__dict__
    for k, v in shipped.items():
        assert k in ours and ours[k] == v, (k, v, ours.get(k))
    assert set(ours) == set(shipped)


def _jape(**over):
    from openea_amd.run.default_args import get_args
    m = JAPE()
    m.set_args(get_args("JAPE", output="/tmp/oea_jape_cpu/", training_data="synthetic/tiny/", dataset_division="f/", **over))
    return m


@pytest.mark.parametrize("over", [dict(alignment_module="mapping"), dict(init="xavier"), dict(neg_sampling="truncated"),
                                  dict(optimizer="Adam"), dict(eval_metric="cosine"), dict(loss_norm="L1"), dict(ent_l2_norm=False),
                                  dict(rel_l2_norm=False), dict(neg_triple_num=0), dict(neg_alpha=-0.1), dict(top_attr_threshold=0.0),
                                  dict(attr_sim_mat_threshold=0.0), dict(attr_sim_mat_beta=0.0)])
def test_init_asserts(over):
    """jape.py:35-50, before any table is made (no GPU here)"""
    m = _jape(**over)
    with pytest.raises(AssertionError):
        m.init()
    assert m.ent_embeds is None


def test_dim_above_the_kernel_limit_is_refused_before_any_table(tiny_kgs):
    from openea_amd.approaches import Attr2Vec
    m = _jape(dim=129)
    with pytest.raises(NotImplementedError, match="129"):
        m.init()
    assert m.ent_embeds is None
    a = Attr2Vec()
    a.set_args(m.args)
    a.set_kgs(tiny_kgs)
    assert a.num_sampled_negs == len(a.selected_attributes) // 5 > 0
    with pytest.raises(NotImplementedError, match="129"):
        a.init()


def test_exports_and_the_reference_method_names():
    from openea_amd import approaches
    assert approaches.JAPE is JAPE and approaches.Attr2Vec.__name__ == "Attr2Vec"
    for name in ("init", "launch_triple_training_1epo", "launch_sim_1epo", "run_attr2vec", "run", "_define_sim_graph"):
        assert callable(getattr(JAPE, name)), name
    for name in ("set_kgs", "set_args", "init", "eval_attribute_embeddings", "eval_kg1_ent_embeddings", "eval_kg2_ent_embeddings",
                 "eval_sim_mat", "eval_sim_csr", "launch_training_1epo", "valid", "test", "run", "save"):
        assert callable(getattr(approaches.Attr2Vec, name)), name
    assert JapeTrainer.fused_epoch is False and "jape.py:136" in approaches.jape.__doc__
