"""RotatE and DistMult without a GPU: a float64 restatement of both losses (CPU torch autograd) against the reference's own graphs
(tests/golden/rotate_distmult_graph.npz, make_rotate_distmult_golden.py), the RotatE restatement against the oracle that the
BootEA_RotatE step is already held to, the shipped run configs and the argument contract.  The GPU tests
(test_rotate_distmult_gpu.py) hold the device steps to these restatements at shapes the finite-difference fixture cannot reach."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rotate_distmult_graph.npz")
ROTATE_VARS = ("re_ent_embeds", "im_ent_embeds", "rel_embeds")
DISTMULT_VARS = ("ent_embeds", "rel_embeds")
CASES = ["rotate_d6_k2", "rotate_d16_k3", "distmult_d5_k1", "distmult_d16_k3"]


def _l2n(x):
    """tf.nn.l2_normalize(x, 1): x * rsqrt(max(sum x^2, 1e-12))"""
    return x * torch.rsqrt(torch.clamp((x * x).sum(1, keepdim=True), min=1e-12))


def _ids(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.long)


def rotate_loss(re, im, rel, pos, neg, gamma, phase_scale, neg_loss_div=1, ent_l2_norm=True, rel_l2_norm=True):
    """rotate.py:61-110 in float64: -sum log sigmoid(gamma - dist+) - sum log sigmoid(dist- - gamma) / neg_loss_div"""
    if ent_l2_norm:
        re, im = _l2n(re), _l2n(im)
    if rel_l2_norm:
        rel = _l2n(rel)

    def dist(tr):
        tr = _ids(tr)
        h, r, t = tr[:, 0], tr[:, 1], tr[:, 2]
        theta = rel[r] * phase_scale
        rr, ir = torch.cos(theta), torch.sin(theta)
        a = re[h] * rr - im[h] * ir - re[t]
        b = re[h] * ir + im[h] * rr - im[t]
        return torch.sqrt(a * a + b * b).sum(1)
    logsig = torch.nn.functional.logsigmoid
    loss = -logsig(gamma - dist(pos)).sum()
    if neg is not None and len(neg):
        loss = loss - logsig(dist(neg) - gamma).sum() / max(int(neg_loss_div), 1)
    return loss


def distmult_loss(ent, rel, pos, neg, ent_l2_norm=True, rel_l2_norm=True):
    """distmult.py:43-58 in float64: the mean over positives (label +1) and negatives (label -1) together"""
    e = _l2n(ent) if ent_l2_norm else ent
    w = _l2n(rel) if rel_l2_norm else rel
    tr = _ids(np.concatenate([np.asarray(pos), np.asarray(neg)]))
    label = torch.cat([torch.ones(len(pos), dtype=torch.float64), -torch.ones(len(neg), dtype=torch.float64)])
    s = (e[tr[:, 0]] * w[tr[:, 1]] * e[tr[:, 2]]).sum(1)
    return torch.nn.functional.softplus(-label * s).mean()


def _grads(fn, tables):
    vs = [torch.tensor(np.asarray(v, np.float64), requires_grad=True) for v in tables]
    loss = fn(*vs)
    return float(loss.detach()), [g.numpy() for g in torch.autograd.grad(loss, vs)]


def rotate_grads(re, im, rel, pos, neg, **kw):
    """-> loss, [d loss / d re, d im, d rel] (float64 numpy)"""
    return _grads(lambda a, b, c: rotate_loss(a, b, c, pos, neg, **kw), (re, im, rel))


def distmult_grads(ent, rel, pos, neg, **kw):
    return _grads(lambda a, b: distmult_loss(a, b, pos, neg, **kw), (ent, rel))


def rotate_reference_step(ent, rel, pos, neg, state, *, gamma, phase_scale, neg_loss_div=1, ent_l2_norm=True, rel_l2_norm=True,
                          optimizer="Adam", lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8):
    """one optimiser step in place on float64 ent = [re; im] [2E, d] and rel [R, d] (the layout of np_oracle.rotate_step);
    tf.train.AdamOptimizer moves every row of a variable every step.  state: {} at first.  -> the batch loss"""
    E = ent.shape[0] // 2
    loss, (g_re, g_im, g_rel) = rotate_grads(ent[:E], ent[E:], rel, pos, neg, gamma=gamma, phase_scale=phase_scale,
                                             neg_loss_div=neg_loss_div, ent_l2_norm=ent_l2_norm, rel_l2_norm=rel_l2_norm)
    pairs = (("ent", ent, np.concatenate([g_re, g_im])), ("rel", rel, g_rel))
    if optimizer == "Adam":
        state["t"] = t = state.get("t", 0) + 1
        lr_t = lr * np.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
        for name, var, g in pairs:
            m = state.setdefault("m_" + name, np.zeros_like(var))
            v = state.setdefault("v_" + name, np.zeros_like(var))
            m *= beta1
            m += (1.0 - beta1) * g
            v *= beta2
            v += (1.0 - beta2) * g * g
            var -= lr_t * m / (np.sqrt(v) + eps)
    else:
        assert optimizer == "SGD"
        for _, var, g in pairs:
            var -= lr * g
    return loss


def distmult_reference_step(tables, accs, pos, neg, lr, optimizer="Adagrad", ent_l2_norm=True, rel_l2_norm=True):
    """one step of (ent, rel) in place (float64); tf.train.AdagradOptimizer, accumulators from 0.1: a zero gradient leaves a row and
    its accumulator unchanged.  -> the batch mean"""
    loss, grads = distmult_grads(tables[0], tables[1], pos, neg, ent_l2_norm=ent_l2_norm, rel_l2_norm=rel_l2_norm)
    for v, a, g in zip(tables, accs, grads):
        if optimizer == "Adagrad":
            a += g * g
            v -= lr * g / np.sqrt(a)
        else:
            v -= lr * g
    return loss


def fixture_case(z, case):
    """-> model, tables, pos, neg, k, keyword arguments of the loss"""
    model = "RotatE" if case.startswith("rotate") else "DistMult"
    names = ROTATE_VARS if model == "RotatE" else DISTMULT_VARS
    tables = [z["%s_var_%s" % (case, n)] for n in names]
    k = int(z[case + "_shape"][3])
    kw = {}
    if model == "RotatE":
        kw = dict(gamma=float(z[case + "_gamma"][0]), phase_scale=float(z[case + "_phase_scale"][0]), neg_loss_div=k)
    return model, names, tables, z[case + "_pos"], z[case + "_neg"], k, kw


@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_reference_graph(case):
    z = np.load(GOLDEN)
    model, names, tables, pos, neg, k, kw = fixture_case(z, case)
    loss, grads = (rotate_grads if model == "RotatE" else distmult_grads)(*tables, pos, neg, **kw)
    ref_loss = z[case + "_loss"][0]
    assert abs(loss - ref_loss) <= 1e-6 * abs(ref_loss)
    for name, g in zip(names, grads):
        ref = z["%s_grad_%s" % (case, name)]
        assert g.shape == ref.shape
        assert np.abs(ref).max() > 0, name
        assert np.abs(g - ref).max() <= 1e-6 * np.abs(ref).max(), name


def test_fixture_covers_the_cases():
    z = np.load(GOLDEN)
    for case in CASES:
        pos, neg = z[case + "_pos"], z[case + "_neg"]
        n_ent, n_rel, d, k = z[case + "_shape"]
        assert len(neg) == k * len(pos)
        assert (np.repeat(pos[:, 1], k) != neg[:, 1]).sum() == 1, case                # a negative with another relation
        assert (pos[:, 0] == pos[:, 2]).any(), case                                   # h == t
        assert len(np.unique(np.concatenate([pos[:, 0], pos[:, 2]]))) < 2 * len(pos), case
        assert max(pos[:, [0, 2]].max(), neg[:, [0, 2]].max()) < n_ent and max(pos[:, 1].max(), neg[:, 1].max()) < n_rel
        for name in (ROTATE_VARS if case.startswith("rotate") else DISTMULT_VARS):
            v = z["%s_var_%s" % (case, name)]
            assert np.array_equal(v, v.astype(np.float32).astype(np.float64)), name   # float32-representable
        assert float(z[case + "_fd_err"][0]) <= 1e-9, case       # the maker's step-size check: what the fp64 GPU test relies on
    assert [tuple(z[c + "_shape"]) for c in CASES] == [(14, 4, 6, 2), (24, 5, 16, 3), (14, 4, 5, 1), (24, 5, 16, 3)]


def _rotate_batch(rng, E, R, n_pos, k):
    """the batch of test_rotate_step_matches_oracle: Zipf relations, one negative that is not a corruption of its positive"""
    pos = np.stack([rng.randint(0, E, n_pos), np.minimum(rng.zipf(1.6, n_pos) - 1, R - 1), rng.randint(0, E, n_pos)], 1).astype(np.int32)
    neg = np.repeat(pos, k, axis=0)
    ch = rng.rand(n_pos * k) < 0.5
    rnd = rng.randint(0, E, n_pos * k)
    neg[ch, 0] = rnd[ch]
    neg[~ch, 2] = rnd[~ch]
    neg[5, 1] = (neg[5, 1] + 1) % R
    return pos, neg


@pytest.mark.parametrize("ent_norm,rel_norm", [(True, True), (True, False)])
def test_rotate_restatement_equals_the_oracle_when_undivided(ent_norm, rel_norm):
    """neg_loss_div = 1 is BootEA_RotatE's loss: three Adam steps equal np_oracle.rotate_step (hand-written gradients), at the
    tolerance the device step is held to against that oracle"""
    from oracle import np_oracle as orc
    rng = np.random.RandomState(17)
    E, R, d, k = 60, 5, 12, 3
    ent = rng.standard_normal((2 * E, d)) / np.sqrt(d)
    rel = rng.standard_normal((R, d)) / np.sqrt(d)
    pos, neg = _rotate_batch(rng, E, R, 40, k)
    kw = dict(gamma=6.0, phase_scale=np.pi / (8.0 / d), ent_l2_norm=ent_norm, rel_l2_norm=rel_norm, optimizer="Adam", lr=0.01)
    e0, r0, s0, e1, r1, s1 = ent.copy(), rel.copy(), {}, ent.copy(), rel.copy(), {}
    ref = sum(orc.rotate_step(e0, r0, pos, neg, s0, **kw) for _ in range(3))
    got = sum(rotate_reference_step(e1, r1, pos, neg, s1, neg_loss_div=1, **kw) for _ in range(3))
    assert abs(got - ref) <= 1e-10 * abs(ref)
    for a, b in ((e1, e0), (r1, r0)):
        assert np.linalg.norm(a - b) <= 1e-9 * np.linalg.norm(b)
    assert np.linalg.norm(e1 - ent) > 1e-3 * np.linalg.norm(ent)


def test_rotate_divisor_weights_the_negative_half_only():
    rng = np.random.RandomState(2)
    E, R, d, k = 30, 4, 8, 5
    ent, rel = rng.standard_normal((2 * E, d)), rng.standard_normal((R, d))
    pos, neg = _rotate_batch(rng, E, R, 12, k)
    kw = dict(gamma=3.0, phase_scale=1.7)
    t = [torch.tensor(x) for x in (ent[:E], ent[E:], rel)]
    whole = float(rotate_loss(*t, pos, neg, neg_loss_div=1, **kw))
    half = float(rotate_loss(*t, pos, None, **kw))
    assert abs(float(rotate_loss(*t, pos, neg, neg_loss_div=k, **kw)) - (half + (whole - half) / k)) <= 1e-12 * whole
    assert float(rotate_loss(*t, pos, neg, neg_loss_div=0, **kw)) == whole


def test_distmult_loss_is_a_mean_over_the_labelled_list():
    rng = np.random.RandomState(4)
    ent, rel = torch.tensor(rng.standard_normal((20, 6))), torch.tensor(rng.standard_normal((3, 6)))
    pos = np.stack([rng.randint(0, 20, 9), rng.randint(0, 3, 9), rng.randint(0, 20, 9)], 1)
    neg = np.repeat(pos, 2, axis=0)
    neg[:, 2] = rng.randint(0, 20, 18)
    one = float(distmult_loss(ent, rel, pos, neg))
    two = float(distmult_loss(ent, rel, np.concatenate([pos, pos]), np.concatenate([neg, neg])))
    assert abs(one - two) <= 1e-14 * one
    perm = rng.permutation(18)
    assert abs(float(distmult_loss(ent, rel, pos[::-1], neg[perm])) - one) <= 1e-14 * one


# run/args/rotate_args_15K.json and rotate_args_100K.json, every key
ROTATE_15K = dict(training_data="../../datasets/", output="../../output/results/", dataset_division="721_5fold",
                  embedding_module="RotatE", alignment_module="sharing", search_module="greedy", dim=100, init="uniform",
                  ent_l2_norm=True, rel_l2_norm=True, neg_sampling="uniform", neg_triple_num=10, gamma=12.0, learning_rate=0.1,
                  optimizer="Adam", max_epoch=2000, batch_size=5000, batch_threads_num=2, test_threads_num=2, ordered=True,
                  start_valid=200, eval_freq=10, stop_metric="hits1", eval_metric="inner", csls=10, top_k=[1, 5, 10, 50],
                  is_save=True, eval_norm=True)
ROTATE_100K = dict(ROTATE_15K, batch_size=20000, batch_threads_num=3, test_threads_num=1)


@pytest.mark.parametrize("scale,expect", [("15K", ROTATE_15K), ("100K", ROTATE_100K)])
def test_rotate_args_match_the_shipped_run_configs(scale, expect):
    from openea_amd.run.default_args import get_args
    assert vars(get_args("RotatE", scale)) == expect


@pytest.mark.parametrize("scale", ["15K", "100K"])
def test_distmult_args_carry_the_simple_values(scale):
    from openea_amd.run.default_args import get_args
    a, s = vars(get_args("DistMult", scale)), vars(get_args("SimplE", scale))
    assert a.pop("embedding_module") == "DistMult" and s.pop("embedding_module") == "SimplE"
    assert a == s
    assert (a["optimizer"], a["learning_rate"], a["neg_triple_num"], a["start_valid"], a["eval_norm"]) == \
        ("Adagrad", 0.01, 1, 10 if scale == "15K" else 50, True)
    assert a["batch_size"] == (5000 if scale == "15K" else 20000)


@pytest.mark.parametrize("name,bad", [("RotatE", dict(init="normal")), ("RotatE", dict(alignment_module="swapping")),
                                      ("RotatE", dict(neg_sampling="truncated")), ("RotatE", dict(optimizer="Adagrad")),
                                      ("RotatE", dict(eval_metric="euclidean")), ("RotatE", dict(gamma=0.0)),
                                      ("DistMult", dict(alignment_module="mapping")), ("DistMult", dict(neg_sampling="truncated")),
                                      ("DistMult", dict(optimizer="Adam")), ("DistMult", dict(optimizer="SGD"))])
def test_init_rejects_each_required_key(name, bad):
    """rotate.py:43-50; DistMult: what the device path needs, Adagrad being what the reference hard-wires.  init() raises before
    any table is made: there is no device here, and no KGs are set"""
    from openea_amd.models import semantic
    from openea_amd.run.default_args import get_args
    m = getattr(semantic, name)()
    m.args = get_args(name)
    m._check_args()
    m.args = get_args(name, **bad)
    with pytest.raises(AssertionError):
        m._check_args()
    with pytest.raises(AssertionError):
        m.init()


def test_one_gpu_and_dim_limits_are_raised_before_any_table(monkeypatch):
    from openea_amd.models import semantic
    from openea_amd.run.default_args import get_args
    m = semantic.DistMult()
    m.args = get_args("DistMult", dim=129)
    with pytest.raises(NotImplementedError, match="dim 129 > 128"):
        m.init()
    for name in ("RotatE", "DistMult"):
        m = getattr(semantic, name)()
        m.args = get_args(name)
        monkeypatch.setattr(type(m), "_dist_group", staticmethod(lambda: object()))
        with pytest.raises(NotImplementedError, match=name + " runs on one GPU"):
            m.init()


def test_exports_and_the_shared_rotate_classes():
    from openea_amd.approaches import bootea_rotate
    from openea_amd.models import semantic
    from openea_amd.models.basic_model import BasicModel
    from openea_amd.models.semantic import rotate_trainer
    for name in ("DistMult", "HolE", "SimplE", "RotatE"):
        assert issubclass(getattr(semantic, name), BasicModel)
    assert semantic.DistMult().metric == "inner"
    for name in ("ComplexEntityTable", "PhaseTable", "RotateTrainer"):            # the old import path still works
        assert getattr(bootea_rotate, name) is getattr(rotate_trainer, name)
    # RotatE overrides neither the epoch loop nor its line; DistMult prints its own
    assert semantic.RotatE.launch_triple_training_1epo is BasicModel.launch_triple_training_1epo
    assert semantic.DistMult.launch_triple_training_1epo is not BasicModel.launch_triple_training_1epo


def test_rotate_cfg_carries_the_divisor_in_the_last_field():
    import ctypes
    from openea_amd import ops
    from openea_amd._lib import RotateCfg
    assert ctypes.sizeof(RotateCfg) == 72 and RotateCfg._fields_[-1] == ("neg_loss_div", ctypes.c_int32)
    assert RotateCfg.neg_loss_div.offset == 68
    assert ops.make_rotate_cfg(12.0, 100).neg_loss_div == 0
    cfg = ops.make_rotate_cfg(12.0, 100, True, True, "Adam", 0.1, neg_loss_div=10)
    assert cfg.neg_loss_div == 10 and cfg.opt_kind == 2 and abs(cfg.phase_scale - np.pi / 0.14) < 1e-12
    assert (ops.SEMANTIC_HOLE, ops.SEMANTIC_SIMPLE, ops.SEMANTIC_DISTMULT) == (0, 1, 2)
