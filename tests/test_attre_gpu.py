"""AttrE's three entry points (csrc/attre_step.hip) on the device.

The character step is held to float64 GRADIENTS per row by the rule of tests/_grads.py: one SGD step with lr = 1.0, before - after
against the float64 restatement (_attre_ref.char_grads) within 4 E32 + 2^-24 |after row|, E32 measured from the float32 run of the
same restatement; the loss within (d + 32) 2^-24 sum |term|.  A problem is built once per process and not written to.

Hinges.  A hinge (margin-based: margin + pos - neg; limited: pos - pos_margin, neg_margin - neg) whose float64 argument lies within
4 (d + 16) 2^-24 (|margin| + pos + neg) of zero may fall on the other side in float32 -- a d-term fp32 sum is that exact -- and
then a whole gradient row differs.  Positives with such an argument get another entity and other negative heads before either
side runs.

d = 1.  A one-column row normalises to +-1, the exact gradient of a normalised table is zero and what the step returns is the
rounding of y^2 = 1 + eta, |eta| < 2^-21, times the gradient that reaches the row, divided by |a| (tests/_grads.one_column_floor).
The gradient one triple sends to a unit row is at most 2 |x| <= 2 (2 + L) (L2; |v| <= sum_p w_p = L) or 1 (L1) per scored triple;
an attribute row gets that from the positive and its k negatives, a character row w_i times that.  Summed over the batch's
references to a row this replaces E32 alone there: 2^-20 sum / |a|."""
import functools
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import _attre_ref as ref  # noqa: E402
import _grads as G  # noqa: E402
from _tol import assert_rows_close  # noqa: E402
from test_attre_cpu import CASES, GOLD, golden_batch, golden_tables  # noqa: E402

N_ENT, N_ATTR = 60, 6              # the last 10 entities and the last attribute are in no triple
ENT_USED, ATTR_USED = 50, 5
MARGINS = dict(margin=1.5, pos_margin=3.0, neg_margin=6.0, balance=1.0)


def _scores(tables, b):
    """float64 scores of the positives [n] and of their negatives [n, k]"""
    ent, attr, chars = (torch.tensor(np.asarray(t, np.float64)) for t in tables)
    pos, k, n = b["pos"], b["k"], len(b["pos"])
    w = torch.tensor(ref.weights(b["value_chars"].shape[1]))
    E, A, C = ref._l2n(ent, b["ent_l2n"]), ref._l2n(attr, b["attr_l2n"]), ref._l2n(chars, b["char_l2n"])
    v = (C[ref._ids(b["value_chars"][pos[:, 2]])] * w[None, :, None]).sum(1)
    wa = A[ref._ids(pos[:, 1])]
    ps = ref._score(E[ref._ids(pos[:, 0])] + wa - v, b["l1"]).numpy()
    ns = ref._score(E[ref._ids(b["neg_heads"])] + wa.repeat_interleave(k, 0) - v.repeat_interleave(k, 0), b["l1"]).numpy().reshape(n, k)
    return ps, ns


def _between_the_middle(x):
    """a float32 value between the two middle scores: half of the hinges on either side"""
    x = np.sort(np.asarray(x).reshape(-1))
    return float(np.float32(0.9 * x[0] if len(x) < 2 else 0.5 * (x[len(x) // 2 - 1] + x[len(x) // 2])))


def _hinge_arguments(tables, b):
    """float64 [n, 1 + k]: the arguments of the batch's hinges and their scale (inf where there is no hinge)"""
    ps, ns = _scores(tables, b)
    n, k = len(ps), b["k"]
    arg, scale = np.full((n, 1 + k), np.inf), np.ones((n, 1 + k))
    if b["loss"] == "margin-based":
        arg[:, 0], scale[:, 0] = b["margin"] + ps - ns[:, 0], abs(b["margin"]) + ps + ns[:, 0]
    elif b["loss"] == "limited":
        arg[:, 0], scale[:, 0] = ps - b["pos_margin"], ps + b["pos_margin"]
        arg[:, 1:], scale[:, 1:] = b["neg_margin"] - ns, ns + b["neg_margin"]
    return arg, scale


@functools.lru_cache(maxsize=None)
def problem(dim, L=5, k=1, loss="margin-based", l1=False, l2n=True, n_pos=37, n_chars=7, margin=None, own_heads=False):
    """tables (float32-representable), a batch of n_pos positives with value rows of their own, the float64 loss and gradients and
    the float32 run.  With six positives or more the batch holds: an entity in two positives, a negative head that is another
    positive's head, a value of all padding, a value with one character twice, two positives sharing an attribute.
    own_heads: every negative head is its positive's head (margin 0: every hinge argument is 0.0 exactly)."""
    rng = np.random.RandomState(1000 * dim + 7 * n_pos + 31 * L + k + 100003 * n_chars + (17 if l1 else 0) + (5 if l2n else 0)
                                + {"margin-based": 0, "logistic": 40000, "limited": 80000}[loss])
    tables = [G.f32(rng.standard_normal((rows, dim)) * 0.5) for rows in (N_ENT, N_ATTR, n_chars)]
    pos = np.stack([rng.randint(0, ENT_USED, n_pos), rng.randint(0, ATTR_USED, n_pos), np.arange(n_pos)], 1).astype(np.int32)
    neg = rng.randint(0, ENT_USED, (n_pos, k)).astype(np.int32)
    value_chars = rng.randint(0, n_chars, (n_pos, L)).astype(np.int32)
    if n_pos >= 6:
        pos[1, 0] = pos[0, 0]
        neg[2, 0] = pos[3, 0]
        value_chars[1] = 0
        value_chars[4] = rng.randint(1, n_chars)            # L >= 2: one character twice (and more)
        pos[5, 1] = pos[4, 1]
    b = dict(pos=pos, neg_heads=neg.reshape(-1), value_chars=value_chars, k=k, loss=loss, l1=l1, ent_l2n=l2n, attr_l2n=l2n, char_l2n=l2n,
             **MARGINS)
    if margin is not None:
        b["margin"] = margin
    if loss == "limited":                    # the scores grow with L, the norm and without l2n: margins between the middle scores
        ps, ns = _scores(tables, b)
        b["pos_margin"], b["neg_margin"] = _between_the_middle(ps), _between_the_middle(ns)
    moved = 0
    if own_heads:
        neg[:] = pos[:, :1]
        b["neg_heads"] = neg.reshape(-1)
    elif loss != "logistic" and (margin is None or abs(margin) < 100):
        for _ in range(30):
            arg, scale = _hinge_arguments(tables, b)
            bad = (np.abs(arg) < 4 * (dim + 16) * G.U24 * scale).any(1)
            if not bad.any():
                break
            moved += int(bad.sum())
            pos[bad, 0] = rng.randint(0, ENT_USED, int(bad.sum()))
            neg[bad] = rng.randint(0, ENT_USED, (int(bad.sum()), k))
            b["neg_heads"] = neg.reshape(-1)
        else:
            raise AssertionError("hinges still on their kink")
        assert 100 * moved < max(n_pos, 100) * 3, moved
    if n_pos >= 6 and not own_heads:
        heads = set(pos[:, 0].tolist())
        assert len(heads) < n_pos and any(h in heads and h != pos[p, 0] for p in range(n_pos) for h in neg[p])
        assert (value_chars == 0).all(1).any() and len(set(pos[:, 1].tolist())) < n_pos
        assert L < 2 or any(len(set(r.tolist())) < L for r in value_chars)
    loss64, g64 = ref.char_grads(tables, b)
    loss32, g32 = ref.char_grads(tables, b, np.float32)
    arg, _ = _hinge_arguments(tables, b)
    finite = np.isfinite(arg)
    active = float((arg[finite] > 0).mean()) if finite.any() else 1.0
    return dict(dim=dim, tables=tables, batch=b, loss64=loss64, g64=g64, loss32=loss32, g32=g32, abs_terms=abs(loss64), active=active,
                moved=moved)


def _floors(p):
    """d = 1 with the normalisation on: the per-row floor of the module docstring for the three tables, else 0.0"""
    b, L = p["batch"], p["batch"]["value_chars"].shape[1]
    if p["dim"] != 1 or not b["ent_l2n"]:
        return [0.0, 0.0, 0.0]
    bound = 1.0 if b["l1"] else 2.0 * (2 + L)
    k, pos = b["k"], b["pos"]
    m_ent = np.bincount(np.concatenate([pos[:, 0], b["neg_heads"]]), minlength=N_ENT) * bound
    m_attr = np.bincount(pos[:, 1], minlength=N_ATTR) * (k + 1) * bound
    m_char = np.zeros(len(p["tables"][2]))
    np.add.at(m_char, b["value_chars"][pos[:, 2]].reshape(-1), np.tile(ref.weights(L), len(pos)) * (k + 1) * bound)
    return [2.0 ** -20 * m / np.maximum(np.abs(t[:, 0]), 1e-6) for m, t in zip((m_ent, m_attr, m_char), p["tables"])]


def _setup(tables, b, dev, optimizer="SGD", lr=1.0, max_pos=None):
    from openea_amd import ops
    dim = tables[0].shape[1]
    e, a, c = (ops.to_table(t, dev=dev) for t in tables)
    adagrad = optimizer == "Adagrad"
    accs = [torch.full_like(t, 0.1) if adagrad else None for t in (e, a, c)]
    cfg = ops.make_step_cfg(loss=b["loss"], loss_norm="L1" if b["l1"] else "L2", margin=b["margin"], pos_margin=b["pos_margin"],
                            neg_margin=b["neg_margin"], balance=b["balance"], ent_l2_norm=b["ent_l2n"], rel_l2_norm=b["attr_l2n"],
                            optimizer=optimizer, lr=lr, neg_group_k=b["k"])
    return dict(e=e, a=a, c=c, accs=accs, cfg=cfg, dim=dim, ws=ops.step_workspace(e.shape[0], a.shape[0], e.shape[1], dev),
                cws=ops.attre_char_workspace(c.shape[0], c.shape[1], max_pos or len(b["pos"]), dev),
                err=torch.zeros(1, dtype=torch.int32, device=dev), loss=torch.zeros(1, dtype=torch.float64, device=dev),
                pos=ops.to_ids(b["pos"], dev), neg=ops.to_ids(b["neg_heads"], dev), values=ops.to_ids(b["value_chars"], dev),
                char_l2n=b["char_l2n"])


def _step(s, char_path=0, n_slabs=0):
    from openea_amd import ops
    ops.attre_char_step(s["e"], s["accs"][0], s["a"], s["accs"][1], s["c"], s["accs"][2], s["dim"], s["values"], s["pos"], s["neg"],
                        s["char_l2n"], s["cfg"], s["ws"], s["cws"], s["err"], s["loss"], char_path=char_path, n_slabs=n_slabs)


def _check(p, s, what, loss=True):
    d, b = p["dim"], p["batch"]
    assert int(s["err"].item()) == 0
    named = [np.zeros(N_ENT, bool), np.zeros(N_ATTR, bool), np.zeros(len(p["tables"][2]), bool)]
    named[0][np.concatenate([b["pos"][:, 0], b["neg_heads"]])] = True
    named[1][b["pos"][:, 1]] = True
    named[2][b["value_chars"][b["pos"][:, 2]].reshape(-1)] = True
    assert not named[0][ENT_USED:].any() and not named[1][ATTR_USED:].any()
    ratios = []
    for i, (name, t0, dev_t, floor) in enumerate(zip(("ent_ce", "attr", "chars"), p["tables"], (s["e"], s["a"], s["c"]), _floors(p))):
        after = dev_t.cpu().numpy()
        before = t0.astype(np.float32)
        assert not after[:, d:].any(), "%s %s: pad columns" % (what, name)
        ratios.append(G.gradient_check("%s %s" % (what, name), before, np.ascontiguousarray(after[:, :d]), p["g64"][i], p["g32"][i], floor))
        assert np.array_equal(after[~named[i], :d], before[~named[i]]), "%s %s: a row no triple names moved" % (what, name)
    assert int(s["ws"][: -8 * 4096].count_nonzero()) == 0, what + ": the step workspace is not clean"
    if loss:
        G.loss_check(what, float(s["loss"].item()), p, d)
    return max(ratios)


def _case(char_path=0, n_slabs=0, **kw):
    from openea_amd import ops
    dev = ops.device()
    p = problem(**kw)
    s = _setup(p["tables"], p["batch"], dev)
    _step(s, char_path, n_slabs)
    torch.cuda.synchronize()
    b = p["batch"]
    what = "AttrE %s %s d=%d L=%d k=%d n=%d C=%d l2n=%d path=%d (%.0f%% active, %d moved)" % (
        b["loss"], "L1" if b["l1"] else "L2", p["dim"], b["value_chars"].shape[1], b["k"], len(b["pos"]), len(p["tables"][2]),
        b["ent_l2n"], char_path, 100 * p["active"], p["moved"])
    _check(p, s, what)
    return p, s


# ---- 1. gradients -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("dim", [1, 2, 3, 64, 65, 75, 100, 127, 128])
def test_gradients_at_edge_dimensions(dim, k):
    _case(dim=dim, k=k, loss="margin-based" if k == 1 else "logistic")


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("L", [1, 5, 10])
def test_gradients_at_literal_lengths(L, k):
    _case(dim=75, L=L, k=k, loss="margin-based" if k == 1 else "limited")


@pytest.mark.parametrize("l2n", [True, False])
@pytest.mark.parametrize("l1", [False, True])
@pytest.mark.parametrize("loss", ["margin-based", "logistic", "limited"])
def test_gradients_of_every_loss_and_norm(loss, l1, l2n):
    p, _ = _case(dim=75, k=1 if loss == "margin-based" else 3, loss=loss, l1=l1, l2n=l2n)
    if loss != "logistic":
        assert 0.05 < p["active"] < 1.0 or not l2n, p["active"]


@pytest.mark.parametrize("n_pos", [1, 3])
def test_gradients_below_one_block(n_pos):
    _case(dim=75, k=3, loss="logistic", n_pos=n_pos)


def test_gradients_past_the_grid_cap():
    """2,048 blocks x 4 waves = 8,192 positives: 8,195 sends three waves of block 0 on a second trip; one slab per CU on the LDS path"""
    _case(dim=6, k=1, loss="margin-based", n_pos=8195)


def test_character_gradient_paths():
    """C = 7 in LDS slabs (one, and five for 37 positives), the same by atomics; C just above the limit takes the atomic path"""
    from openea_amd import ops
    for path, slabs in ((ops.ATTRE_PATH_LDS, 1), (ops.ATTRE_PATH_LDS, 5), (ops.ATTRE_PATH_ATOMIC, 0)):
        _case(char_path=path, n_slabs=slabs, dim=75, k=3, loss="logistic")
    limit = ops.attre_lds_chars(76)
    assert limit == 128 * 1024 // (76 * (8 if ops.deterministic() else 4))
    p = problem(dim=75, k=3, loss="logistic", n_chars=limit + 1)
    _case(dim=75, k=3, loss="logistic", n_chars=limit + 1)
    s = _setup(p["tables"], p["batch"], ops.device())
    with pytest.raises(ops.OpenEAHipError):
        _step(s, ops.ATTRE_PATH_LDS)
    _case(dim=75, k=3, loss="logistic", n_chars=limit)             # the largest slab


def test_margin_hinges():
    from openea_amd import ops
    p, _ = _case(dim=75, margin=1000.0)
    assert p["active"] == 1.0
    for kw in (dict(margin=-1000.0), dict(margin=0.0, own_heads=True)):         # all inactive; every argument exactly zero
        p = problem(dim=75, **kw)
        arg, _ = _hinge_arguments(p["tables"], p["batch"])
        assert (arg[:, 0] == 0).all() if "own_heads" in kw else (arg[:, 0] < 0).all()
        assert p["loss64"] == 0 and not any(g.any() for g in p["g64"])
        s = _setup(p["tables"], p["batch"], ops.device())
        _step(s)
        torch.cuda.synchronize()
        for t0, t in zip(p["tables"], (s["e"], s["a"], s["c"])):
            assert np.array_equal(t.cpu().numpy()[:, :75], t0.astype(np.float32))
        assert float(s["loss"].item()) == 0.0 and int(s["ws"][: -8 * 4096].count_nonzero()) == 0


# ---- 2. the reference graph, Adagrad ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,loss,k,norm,d", CASES)
def test_step_equals_reference_graph(tag, loss, k, norm, d):
    from openea_amd import ops
    case = "%s_%s_d%d" % (tag, norm, d)
    b = golden_batch(loss, k, norm, d)
    b = dict(b, pos=b["pos"].astype(np.int32), neg_heads=b["neg_heads"].astype(np.int32), value_chars=b["value_chars"].astype(np.int32))
    tables = golden_tables(d)
    s = _setup(tables, b, ops.device())
    _step(s)
    torch.cuda.synchronize()
    value = GOLD[case + "_loss"][0]
    assert abs(float(s["loss"].item()) - value) <= (d + 32) * G.U24 * value
    for name, t0, t in zip(("ent_embeds_ce", "attr_embeds", "char_embeds"), tables, (s["e"], s["a"], s["c"])):
        got = t0.astype(np.float32).astype(np.float64) - t.cpu().numpy()[:, :d]
        assert_rows_close(got, GOLD["%s_grad_%s" % (case, name)], "%s %s" % (case, name))


@pytest.mark.parametrize("loss,k", [("margin-based", 1), ("limited", 3)])
def test_adagrad_three_steps(loss, k):
    from openea_amd import ops
    p = problem(dim=75, k=k, loss=loss)
    s = _setup(p["tables"], p["batch"], ops.device(), "Adagrad", 0.05)
    tables, accs = [t.copy() for t in p["tables"]], [np.full(t.shape, 0.1) for t in p["tables"]]
    total = 0.0
    for _ in range(3):
        _step(s)
        value, grads = ref.char_grads(tables, p["batch"])
        total += value
        tables, accs = ref.optimiser_step(tables, grads, accs, "Adagrad", 0.05)
    torch.cuda.synchronize()
    assert abs(float(s["loss"].item()) - total) <= 1e-4 * total
    for name, t, acc, want, want_acc in zip(("ent_ce", "attr", "chars"), (s["e"], s["a"], s["c"]), s["accs"], tables, accs):
        assert_rows_close(t.cpu().numpy()[:, :75], want, "Adagrad x3 %s %s" % (loss, name))
        assert_rows_close(acc.cpu().numpy()[:, :75], want_acc, "Adagrad x3 %s %s accumulator" % (loss, name))


# ---- 3. the joint epoch ----------------------------------------------------------------------------------------------------------------
def _joint_tables(rng, n, d):
    return G.f32(rng.standard_normal((n, d)) * 0.5), G.f32(rng.standard_normal((n, d)) * 0.5)


def _joint(ent, ce, dev, optimizer, lr, steps, calls=1, l2n=True, count=None):
    from openea_amd import ops
    d = ent.shape[1]
    e, c = ops.to_table(ent, dev=dev), ops.to_table(ce, dev=dev)
    accs = (torch.full_like(e, 0.1), torch.full_like(c, 0.1)) if optimizer == "Adagrad" else (None, None)
    loss = torch.zeros(steps * calls, dtype=torch.float64, device=dev)
    for i in range(calls):
        ops.attre_joint_epoch(e, accs[0], c, accs[1], d, l2n, optimizer, lr, steps, loss[i * steps:],
                              None if count is None else ops.to_ids(count, dev))
    torch.cuda.synchronize()
    return e.cpu().numpy(), c.cpu().numpy(), loss.cpu().numpy(), accs


@pytest.mark.parametrize("optimizer", ["SGD", "Adagrad"])
@pytest.mark.parametrize("d", [3, 100])
def test_joint_epoch_equals_single_steps_bit_for_bit(d, optimizer):
    from openea_amd import ops
    dev = ops.device()
    ent, ce = _joint_tables(np.random.RandomState(d), 301, d)
    e4, c4, l4, a4 = _joint(ent, ce, dev, optimizer, 0.3, 4)
    e1, c1, l1, a1 = _joint(ent, ce, dev, optimizer, 0.3, 1, calls=4)
    assert np.array_equal(e4, e1) and np.array_equal(c4, c1) and (e4[:, :d] != ent.astype(np.float32)).any()
    assert np.allclose(l4, l1, rtol=1e-12, atol=0) and (np.diff(l4) < 0).all()
    if optimizer == "Adagrad":
        assert all(torch.equal(x, y) for x, y in zip(a4, a1))
    e40, c40, l40, _ = _joint(ent, ce, dev, optimizer, 0.3, 40)                 # more steps than one launch holds
    e5, c5, l5, _ = _joint(ent, ce, dev, optimizer, 0.3, 8, calls=5)
    assert np.array_equal(e40, e5) and np.array_equal(c40, c5) and np.allclose(l40, l5, rtol=1e-12, atol=0)


@pytest.mark.parametrize("n,d", [(1, 75), (301, 1), (301, 75), (301, 128), (8195, 6)])
def test_joint_gradients(n, d):
    """one SGD step at lr = 1.0 against float64; row 3 of ent is all zero (the clamp: l2n(0) = 0, its gradient -yb / 1e-6);
    8,195 rows lie past the grid cap of 2,048 x 4.  From 301 rows on the entity list names every seventh row twice and leaves
    rows 5 and 6 out."""
    from openea_amd import ops
    rng = np.random.RandomState(n + d)
    ent, ce = _joint_tables(rng, n, d)
    count = None
    if n > 3:
        ent[3] = 0.0
        count = np.ones(n, np.int32)
        count[::7] = 2
        count[5:7] = 0
    entities = None if count is None else np.repeat(np.arange(n), count)
    loss64, g64 = ref.joint_grads(ent, ce, True, entities=entities)
    _, g32 = ref.joint_grads(ent, ce, True, np.float32, entities=entities)
    e, c, loss, _ = _joint(ent, ce, ops.device(), "SGD", 1.0, 1, count=count)
    if count is not None:
        assert np.array_equal(e[5:7, :d], ent[5:7].astype(np.float32)) and np.array_equal(c[5:7, :d], ce[5:7].astype(np.float32))
    for name, t0, t, a, b in zip(("ent", "ent_ce"), (ent, ce), (e, c), g64, g32):
        floor = 2.0 ** -19 / np.maximum(np.abs(t0[:, 0]), 1e-6) if d == 1 else 0.0        # at most two unit rows reach the row (see above)
        assert not t[:, d:].any()
        G.gradient_check("joint n=%d d=%d %s" % (n, d, name), t0.astype(np.float32), np.ascontiguousarray(t[:, :d]), a, b, floor)
    assert abs(loss[0] - loss64) <= (d + 32) * G.U24 * 2 * n
    if n > 3:
        assert np.abs(g64[0][3]).max() > 1e3                                       # the clamped row's gradient is the large one


# ---- 4. the sampler --------------------------------------------------------------------------------------------------------------------
def test_sampler_equals_its_restatement():
    from openea_amd import ops
    from test_attre_cpu import _sides
    dev = ops.device()
    rng = np.random.RandomState(9)
    n_ent = 500
    perm = rng.permutation(n_ent)
    lists, poss = _sides(perm[:230], perm[230:], n_ent)
    n, k, split = 3001, 3, 1400
    pos = np.zeros((n, 3), np.int32)
    pos[:split, 0], pos[split:, 0] = rng.choice(lists[0], split), rng.choice(lists[1], n - split)
    d = [ops.to_ids(x, dev) for x in (lists[0], poss[0], lists[1], poss[1])]
    pd = ops.to_ids(pos, dev)
    for seed, step in ((5, 0), (2 ** 40 + 17, 123456)):
        got = ops.attre_sample_heads(pd, split, k, d[0], d[1], d[2], d[3], seed, step).cpu().numpy()
        want = ref.sample_heads(pos, split, k, lists, poss, seed, step)
        assert np.array_equal(got, want) and (got.reshape(n, k) != pos[:, :1]).all()
    part = ops.attre_sample_heads(pd[1000:], split - 1000, k, d[0], d[1], d[2], d[3], 5, 0, pos_offset=1000).cpu().numpy()
    assert np.array_equal(part, ref.sample_heads(pos, split, k, lists, poss, 5, 0)[1000 * k:])       # a split batch
    one = ops.to_ids(lists[0][:1], dev)
    out = torch.full((n * k,), -7, dtype=torch.int32, device=dev)
    with pytest.raises(ops.OpenEAHipError):
        ops.attre_sample_heads(pd, split, k, one, d[1], d[2], d[3], 5, 0, out=out)
    with pytest.raises(ops.OpenEAHipError):
        ops.attre_sample_heads(pd, split, k, d[0], d[1], one, d[3], 5, 0, out=out)
    with pytest.raises(ops.OpenEAHipError):
        ops.attre_sample_heads(pd, split, 0, d[0], d[1], d[2], d[3], 5, 0, out=out)
    assert (out == -7).all()
    ops.attre_sample_heads(pd[:split], split, k, d[0], d[1], one, d[3], 5, 0, out=out)              # a side not in use may be short


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched():
    from openea_amd import ops
    dev = ops.device()
    p = problem(dim=75, k=3, loss="logistic")
    b = p["batch"]

    def fresh(**over):
        s = _setup(p["tables"], dict(b, **over), dev)
        s["loss"].fill_(-3.0)
        s["before"] = [t.clone() for t in (s["e"], s["a"], s["c"])]
        return s

    def untouched(s, err=0):
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(s["before"], (s["e"], s["a"], s["c"])))
        assert float(s["loss"].item()) == -3.0 and int(s["err"].item()) == err
        assert int(s["ws"][: -8 * 4096].count_nonzero()) == 0

    for bad in ("Adam", "Adadelta"):
        s = fresh()
        s["cfg"] = ops.make_step_cfg(loss="logistic", optimizer=bad, lr=1.0, neg_group_k=3)
        with pytest.raises(ops.OpenEAHipError, match="-4"):
            _step(s)
        untouched(s)
    s = fresh()
    s["neg"] = s["neg"][:-1]                                    # n_neg != k n_pos
    with pytest.raises(ops.OpenEAHipError):
        _step(s)
    untouched(s)
    s = fresh(loss="margin-based")                              # margin-based with k = 3
    with pytest.raises(ops.OpenEAHipError):
        _step(s)
    untouched(s)
    s = fresh()
    s["cws"] = s["cws"][:64]                                    # workspace too small
    with pytest.raises(ops.OpenEAHipError):
        _step(s)
    untouched(s)
    s = fresh()
    s["values"] = torch.zeros((len(b["pos"]), 33), dtype=torch.int32, device=dev)      # literal_len 33
    with pytest.raises(ops.OpenEAHipError):
        _step(s)
    untouched(s)
    wide = [G.f32(np.ones((rows, 129))) for rows in (N_ENT, N_ATTR, 7)]               # dim 129
    s = _setup(wide, b, dev)
    s["loss"].fill_(-3.0)
    s["before"] = [t.clone() for t in (s["e"], s["a"], s["c"])]
    with pytest.raises(ops.OpenEAHipError, match="-4"):
        _step(s)
    untouched(s)
    # ids the check kernel finds: a character id outside the table, then a value row outside value_chars
    s = fresh()
    s["values"] = s["values"].clone()
    s["values"][5, 2] = 7
    _step(s)
    untouched(s, err=1)
    with pytest.raises(ops.OpenEAHipError):
        ops.attre_check(s["err"])
    s = fresh()
    s["pos"] = s["pos"].clone()
    s["pos"][4, 2] = len(b["pos"])
    _step(s)
    untouched(s, err=2)
    # the joint epoch
    e, c = ops.to_table(p["tables"][0], dev=dev), ops.to_table(p["tables"][0] * 2, dev=dev)
    e0, c0 = e.clone(), c.clone()
    loss = torch.full((2,), -3.0, dtype=torch.float64, device=dev)
    for kw in (dict(optimizer="Adam"), dict(optimizer="Adagrad"), dict(steps=0)):      # Adagrad without accumulators
        with pytest.raises(ops.OpenEAHipError):
            ops.attre_joint_epoch(e, None, c, None, 75, True, kw.get("optimizer", "SGD"), 0.1, kw.get("steps", 2), loss)
    torch.cuda.synchronize()
    assert torch.equal(e, e0) and torch.equal(c, c0) and (loss == -3.0).all()


# ---- 6. the fixed-point build ----------------------------------------------------------------------------------------------------------
DET_WORKER = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.environ["OEA_ROOT"]); sys.path.insert(0, os.path.join(os.environ["OEA_ROOT"], "tests"))
import torch
from openea_amd import ops
import test_attre_gpu as T
assert ops.deterministic()
dev = ops.device()
p = T.problem(dim=75, k=3, loss="logistic", n_pos=2000)
runs = []
for _ in range(2):
    s = T._setup(p["tables"], p["batch"], dev, "Adagrad", 0.05)
    for _ in range(2):
        T._step(s, ops.ATTRE_PATH_LDS)
    torch.cuda.synchronize()
    runs.append([t.cpu().numpy() for t in (s["e"], s["a"], s["c"])] + [a.cpu().numpy() for a in s["accs"]] + [s["loss"].cpu().numpy()])
other = [name for name, x, y in zip(("e", "a", "c", "e_acc", "a_acc", "c_acc"), *runs) if not np.array_equal(x, y)]
assert not other, "the fixed-point build gave other bits in " + ", ".join(other)
# the loss is a double that the blocks add with atomics in the order they finish: equal to rounding, not to the bit
assert abs(runs[0][6][0] - runs[1][6][0]) <= 1e-12 * abs(runs[0][6][0]), (runs[0][6], runs[1][6])
np.savez(os.environ["OEA_OUT"], e=runs[0][0], a=runs[0][1], c=runs[0][2])
print("RESULT done")
'''


def test_fixed_point_build_repeats_its_bits(tmp_path):
    """two Adagrad steps of 2,000 positives (125 slabs) twice in libopenea_hip_det.so: the same bits, and the float64 replay"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "det.npz")
    run = subprocess.run([sys.executable, "-c", DET_WORKER], env=dict(os.environ, OEA_ROOT=root, OEA_STEP_DETERMINISTIC="1", OEA_OUT=out),
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "RESULT done" in run.stdout, run.stderr[-2000:]
    p = problem(dim=75, k=3, loss="logistic", n_pos=2000)
    tables, accs = [t.copy() for t in p["tables"]], [np.full(t.shape, 0.1) for t in p["tables"]]
    for _ in range(2):
        tables, accs = ref.optimiser_step(tables, ref.char_grads(tables, p["batch"])[1], accs, "Adagrad", 0.05)
    z = np.load(out)
    for name, want in zip("eac", tables):
        assert_rows_close(z[name][:, :75], want, "fixed-point build, table " + name)


# ---- 7. end to end -----------------------------------------------------------------------------------------------------------------------
def _model(**over):
    from openea_amd.approaches import AttrE
    from openea_amd.modules.load.synth import make_kgs
    from openea_amd.run.default_args import get_args
    m = AttrE()
    m.set_args(get_args("AttrE", output="/tmp/oea_attre_gpu/", training_data="synthetic/tiny/", dataset_division="f/", dim=16,
                        batch_size=500, max_epoch=3, start_valid=100, **over))
    m.set_kgs(make_kgs("tiny", mode="sharing", seed=0, attributes=True, string_values=True))
    m.init()
    return m


def test_attre_end_to_end(capsys):
    m = _model()
    m.run()
    out = capsys.readouterr().out
    number = r"(-?\d+\.\d{4})"
    for pattern in (r"epoch (\d+), avg\. triple loss: %s, cost time: %ss" % (number, number),
                    r"epoch (\d+), CE, avg\. triple loss: %s, cost time: %ss" % (number, number),
                    r"epoch (\d+), joint learning loss: %s, time: %ss" % (number, number)):
        found = re.findall(pattern, out)
        assert [int(f[0]) for f in found] == [1, 2, 3], (pattern, out)
        assert all(np.isfinite(float(f[1])) for f in found)
    assert "Training ends. Total time = " in out


@pytest.mark.parametrize("optimizer", ["SGD", "Adagrad"])
def test_attre_epoch_equals_the_replay(optimizer):
    """the character and the joint epoch of the first epoch against the float64 replay of the same batches and negatives"""
    m = _model(optimizer=optimizer)
    a = m.args
    d, b, k = a.dim, a.batch_size, a.neg_triple_num
    m.launch_triple_training_1epo(1, 6, None, None, None, None)
    raw = lambda t: t.var.cpu().numpy()[:, :d].astype(np.float64)          # noqa: E731
    tables = [raw(m.ent_embeds_ce), raw(m.attr_embeds), raw(m.char_embeds)]
    ent = raw(m.ent_embeds)
    steps = int(np.ceil((len(m.attribute_triples_list1) + len(m.attribute_triples_list2)) / b))
    ce_loss = m.launch_triple_training_1epo_ce(1, steps, None, None)
    pos_all, neg_all = m._attr_dall.cpu().numpy(), m._attr_negs.cpu().numpy()
    assert steps == 7 and pos_all.shape == (steps * b, 3)
    batch = dict(value_chars=m.value_id_char_ids, k=k, loss=a.loss, l1=a.loss_norm == "L1", margin=a.margin, pos_margin=0.0,
                 neg_margin=0.0, balance=1.0, ent_l2n=True, attr_l2n=True, char_l2n=True)
    accs, total = [np.full(t.shape, 0.1) for t in tables], 0.0
    for s in range(steps):
        bs = dict(batch, pos=pos_all[s * b:(s + 1) * b], neg_heads=neg_all[s * b * k:(s + 1) * b * k])
        assert (bs["neg_heads"].reshape(b, k) != bs["pos"][:, :1]).all()
        value, grads = ref.char_grads(tables, bs)
        total += value
        tables, accs = ref.optimiser_step(tables, grads, accs, optimizer, a.learning_rate)
    assert abs(ce_loss - total / (steps * b)) <= 1e-4 * abs(total / (steps * b))
    for name, t, want in zip(("ent_embeds_ce", "attr_embeds", "char_embeds"), (m.ent_embeds_ce, m.attr_embeds, m.char_embeds), tables):
        assert_rows_close(raw(t), want, "character epoch (%s) %s" % (optimizer, name))
    entities = list(m.kgs.kg1.entities_list + m.kgs.kg2.entities_list)
    joint_loss = m.launch_joint_training_1epo(1, entities)
    pair, accs, total = [ent, tables[0]], [np.full(ent.shape, 0.1)] * 2, 0.0
    joint_steps = int(np.ceil(len(entities) / b))
    assert joint_steps == 2 and len(set(entities)) < len(entities)             # the sharing alignment: training pairs are one id
    for _ in range(joint_steps):
        value, grads = ref.joint_grads(pair[0], pair[1], True, entities=entities)
        total += value
        pair, accs = ref.optimiser_step(pair, grads, accs, optimizer, a.learning_rate)
    assert abs(joint_loss - total / (joint_steps * len(entities))) <= 1e-4
    assert_rows_close(raw(m.ent_embeds), pair[0], "joint epoch (%s) ent_embeds" % optimizer)
    assert_rows_close(raw(m.ent_embeds_ce), pair[1], "joint epoch (%s) ent_embeds_ce" % optimizer)
