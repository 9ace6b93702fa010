"""RotatE and DistMult on the device (oea_rotate_step with neg_loss_div, csrc/rotate_step.hip; oea_semantic_step with
OEA_SEMANTIC_DISTMULT, csrc/semantic_step.hip): against the reference's own graphs (tests/golden/rotate_distmult_graph.npz),
against the float64 restatements of test_rotate_distmult_cpu.py at shapes the fixture cannot reach, run to run in the
fixed-point build, the configurations the steps refuse, and end to end through the two model classes."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_rotate_distmult_cpu import (CASES, GOLDEN, _rotate_batch, distmult_reference_step, fixture_case,  # noqa: E402
                                      rotate_reference_step)
from test_semantic_gpu import _xavier, _zipf_batch  # noqa: E402


# ---- helpers ---------------------------------------------------------------------------------------------------------------
def _rotate_setup(ent, rel, d, dev, **cfg_kw):
    from openea_amd import ops
    te, tr = ops.to_table64(ent, dev), ops.to_table64(rel, dev)
    cfg = ops.make_rotate_cfg(**cfg_kw)
    opt = cfg_kw["optimizer"]
    return dict(e=te, r=tr, se=ops.rotate_state(te, opt), sr=ops.rotate_state(tr, opt), cfg=cfg, d=d,
                ws=ops.rotate_workspace(ent.shape[0] // 2, rel.shape[0], te.shape[1], dev),
                loss=torch.zeros(1, dtype=torch.float64, device=dev))


def _rotate_steps(s, pos, neg, k, steps, split=False):
    from openea_amd import ops
    for step in range(steps):
        s["cfg"].t = step + 1
        for phase in ((ops.PHASE_GRAD, ops.PHASE_APPLY) if split else (ops.PHASE_BOTH,)):
            ops.rotate_step(s["e"], s["se"], s["r"], s["sr"], s["d"], pos, neg, k, s["cfg"], s["ws"], s["loss"], phase=phase)


def _dm_setup(tables, optimizer, dev, k=1, lr=0.01):
    from openea_amd import ops
    e, r = ops.to_table(tables[0], dev=dev), ops.to_table(tables[1], dev=dev)
    cfg = ops.make_step_cfg(loss="margin-based", optimizer=optimizer, lr=lr, neg_group_k=k)
    accs = [torch.full_like(t, 0.1) for t in (e, r)] if optimizer == "Adagrad" else [None, None]
    return dict(kind=ops.SEMANTIC_DISTMULT, e=e, r=r, accs=accs, cfg=cfg, d=tables[0].shape[1],
                ws=ops.step_workspace(e.shape[0], r.shape[0], e.shape[1], dev), loss=torch.zeros(1, dtype=torch.float64, device=dev))


def _dm_step(s, pos, neg):
    from openea_amd import ops
    ops.semantic_step(s["kind"], s["e"], s["accs"][0], s["r"], s["accs"][1], s["d"], pos, neg, s["cfg"], s["ws"], s["loss"])


# ---- 1. the reference's graphs, one SGD step ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_sgd_step_equals_reference_graph(case):
    """DistMult (fp32): 2e-5 on the loss, 1e-3 of the largest gradient entry, as test_semantic_gpu.py holds HolE and SimplE.
    RotatE (fp64): 1e-8 relative on both.  The fixture's maker extrapolates central differences at two step sizes and checks
    them against the next coarser pair; the largest disagreement it reports is 1.9e-10 of the largest gradient entry (rotate_d16_k3;
    6.6e-11 for rotate_d6_k2), so the differences are finer than 1e-8 and that bound stands."""
    from openea_amd import ops
    dev = ops.device()
    z = np.load(GOLDEN)
    model, names, tables, pos, neg, k, kw = fixture_case(z, case)
    lr = 0.01
    dpos, dneg = ops.to_ids(pos, dev), ops.to_ids(neg, dev)
    ref_loss = float(z[case + "_loss"][0])
    if model == "RotatE":
        d = tables[0].shape[1]
        s = _rotate_setup(np.concatenate(tables[:2]), tables[2], d, dev, gamma=kw["gamma"], dim=d, ent_l2_norm=True,
                          rel_l2_norm=True, optimizer="SGD", lr=lr, neg_loss_div=k)
        assert abs(s["cfg"].phase_scale - kw["phase_scale"]) <= 1e-12 * kw["phase_scale"]
        _rotate_steps(s, dpos, dneg, k, 1)
        E = tables[0].shape[0]
        ent = s["e"][:, :d].cpu().numpy()
        got = [ent[:E], ent[E:], s["r"][:, :d].cpu().numpy()]
        before = tables
        tol_loss, tol_grad = 1e-8, 1e-8
    else:
        s = _dm_setup(tables, "SGD", dev, k=k, lr=lr)
        _dm_step(s, dpos, dneg)
        d = s["d"]
        got = [s["e"][:, :d].cpu().numpy(), s["r"][:, :d].cpu().numpy()]
        before = [t.astype(np.float32).astype(np.float64) for t in tables]
        tol_loss, tol_grad = 2e-5, 1e-3
    loss = float(s["loss"].item())
    print("%s: loss %.12g (fixture %.12g, relative %.3g)" % (case, loss, ref_loss, abs(loss - ref_loss) / abs(ref_loss)))
    worst = {}
    for name, b, a in zip(names, before, got):
        g = (b - a) / lr                                                  # SGD: the update IS lr * gradient
        ref = z["%s_grad_%s" % (case, name)]
        worst[name] = np.abs(g - ref).max() / np.abs(ref).max()
        print("%s: %s gradient off by %.3g of its largest entry" % (case, name, worst[name]))
    assert abs(loss - ref_loss) <= tol_loss * abs(ref_loss)
    for name in names:
        assert worst[name] <= tol_grad, name


# ---- 2. RotatE: the negatives' half divided by k ----------------------------------------------------------------------------
def _rotate_inputs(d, k):
    rng = np.random.RandomState(1000 + d + k)
    E, R, n_pos = 400, 9, 350
    ent = rng.standard_normal((2 * E, d)) / np.sqrt(d)
    rel = rng.standard_normal((R, d)) / np.sqrt(d)
    pos, neg = _rotate_batch(rng, E, R, n_pos, k)
    return E, R, ent, rel, pos, neg


def _assert_rotate_close(s, d, ref_loss, e_ref, r_ref, what):
    loss = float(s["loss"].item())
    devs = [np.linalg.norm(got[:, :d].cpu().numpy() - ref) / np.linalg.norm(ref) for got, ref in ((s["e"], e_ref), (s["r"], r_ref))]
    print("%s: loss relative %.3g, tables relative %.3g / %.3g" % (what, abs(loss - ref_loss) / abs(ref_loss), devs[0], devs[1]))
    assert abs(loss - ref_loss) <= 1e-10 * abs(ref_loss), what
    assert max(devs) <= 1e-9, what
    for t in (s["e"], s["r"]):
        assert float(t[:, d:].abs().sum()) == 0.0, what                    # pad columns
    assert int(s["ws"][: -8 * 4096].count_nonzero()) == 0, what            # all but the loss partials is left zeroed


@pytest.mark.parametrize("d,k", [(100, 10), (75, 3), (32, 17), (300, 2)])
def test_rotate_weighted_negatives_equal_restatement(d, k):
    """three Adam steps with neg_loss_div = k against rotate_reference_step, whole and split into GRAD / APPLY; k = 17 spreads a
    family over two 16-triple chunks, d = 300 runs without the register accumulation of the family rows, one negative has a
    relation of its own.  neg_loss_div 0 and 1 keep the old meaning: np_oracle.rotate_step at the same tolerance."""
    from openea_amd import ops
    from oracle import np_oracle as orc
    dev = ops.device()
    E, R, ent, rel, pos, neg = _rotate_inputs(d, k)
    kw = dict(gamma=6.0, ent_l2_norm=True, rel_l2_norm=True, optimizer="Adam", lr=0.01)
    dpos, dneg = ops.to_ids(pos, dev), ops.to_ids(neg, dev)
    e_ref, r_ref, st = ent.copy(), rel.copy(), {}
    ref_loss = sum(rotate_reference_step(e_ref, r_ref, pos, neg, st, phase_scale=np.pi / (8.0 / d), neg_loss_div=k, **kw)
                   for _ in range(3))
    for split in (False, True):
        s = _rotate_setup(ent, rel, d, dev, dim=d, neg_loss_div=k, **kw)
        _rotate_steps(s, dpos, dneg, k, 3, split=split)
        _assert_rotate_close(s, d, ref_loss, e_ref, r_ref, "d=%d k=%d neg_loss_div=%d split=%s" % (d, k, k, split))
    e_old, r_old, st = ent.copy(), rel.copy(), {}
    old_loss = sum(orc.rotate_step(e_old, r_old, pos, neg, st, phase_scale=np.pi / (8.0 / d), **kw) for _ in range(3))
    # the two references are thousands of tolerances apart in the entity tables (8.7e-6 relative at d = 300, more elsewhere; the
    # loss alone would not tell them apart at d = 300, where gamma = 6 leaves the negatives 7e-12 of it): no run can meet both
    assert np.linalg.norm(e_old - e_ref) > 1e3 * 1e-9 * np.linalg.norm(e_ref)
    for div in (0, 1):
        s = _rotate_setup(ent, rel, d, dev, dim=d, neg_loss_div=div, **kw)
        _rotate_steps(s, dpos, dneg, k, 3)
        _assert_rotate_close(s, d, old_loss, e_old, r_old, "d=%d k=%d neg_loss_div=%d" % (d, k, div))


def test_rotate_negative_divisor_is_refused():
    from openea_amd import ops
    from openea_amd._lib import OpenEAHipError
    dev = ops.device()
    d, k = 32, 3
    E, R, ent, rel, pos, neg = _rotate_inputs(d, k)
    s = _rotate_setup(ent, rel, d, dev, gamma=6.0, dim=d, ent_l2_norm=True, rel_l2_norm=True, optimizer="Adam", lr=0.01,
                      neg_loss_div=-1)
    e0, r0, se0 = s["e"].clone(), s["r"].clone(), s["se"].clone()
    with pytest.raises(OpenEAHipError):
        _rotate_steps(s, ops.to_ids(pos, dev), ops.to_ids(neg, dev), k, 1)
    torch.cuda.synchronize()
    assert torch.equal(s["e"], e0) and torch.equal(s["r"], r0) and torch.equal(s["se"], se0)
    assert float(s["loss"].item()) == 0.0 and int(s["ws"].count_nonzero()) == 0


# ---- 3. DistMult: Adagrad against the restatement ------------------------------------------------------------------------------
DM_E, DM_R, DM_N = 3000, 40, 700


@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("dim", [8, 75, 100, 128])
def test_distmult_adagrad_steps_equal_restatement(dim, k):
    """three Adagrad steps; dim = 75 has ld != dim, dim > 64 uses the second column of a lane pair's flush.  Rows no triple refers
    to keep their bits and their accumulators stay at 0.1.

    The loss is a mean over N = 700 (k + 1) triples, so even at the learning rate of 1.0 used here a row moves by about 1e-5 a
    step and the row tolerance of _tol alone would pass a wrong gradient.  The movement itself is therefore held as well:
    |(got - start) - (ref - start)| <= 1e-3 |ref - start| (the fp32 gradient tolerance of the fixture test) + 1.5 * 2^-23 |start|
    (three roundings of a table entry to fp32, half an ulp each), in the Frobenius norm over the rows in use.  (At lr = 0.01 the
    rounding term would be twenty times the gradient term and hide a gradient that is 2 % off.)"""
    from _tol import assert_rows_close
    from openea_amd import ops
    dev = ops.device()
    rng = np.random.RandomState(dim + 1000 * k)
    tables = [_xavier(rng, DM_E, dim), _xavier(rng, DM_R, dim)]
    lr = 1.0
    s = _dm_setup(tables, "Adagrad", dev, k=k, lr=lr)
    ref, accs = [t.copy() for t in tables], [np.full_like(t, 0.1) for t in tables]
    loss_ref = 0.0
    for _ in range(3):
        pos, neg = _zipf_batch(rng, DM_E, DM_R, DM_N, k)
        loss_ref += distmult_reference_step(ref, accs, pos, neg, lr)
        _dm_step(s, ops.to_ids(pos, dev), ops.to_ids(neg, dev))
    loss = float(s["loss"].item())
    print("dim=%d k=%d: loss %.9g (restatement %.9g, relative %.3g)" % (dim, k, loss, loss_ref, abs(loss - loss_ref) / loss_ref))
    assert abs(loss - loss_ref) <= 1e-4 * abs(loss_ref)
    got = [s["e"][:, :dim].cpu().numpy(), s["r"][:, :dim].cpu().numpy()]
    got_acc = [s["accs"][0][:, :dim].cpu().numpy(), s["accs"][1][:, :dim].cpu().numpy()]
    for i, (g, r) in enumerate(zip(got, ref)):
        assert_rows_close(g, r, "DistMult d=%d k=%d table %d" % (dim, k, i))
    for i, (g, r) in enumerate(zip(got_acc, accs)):
        assert_rows_close(g, r, "DistMult d=%d k=%d accumulator %d" % (dim, k, i))
    for i, (g, a, r, t0) in enumerate(zip(got, got_acc, ref, tables)):
        tail = 100 if i == 0 else 4
        assert np.array_equal(g[-tail:], t0[-tail:].astype(np.float32)), i
        assert (a[-tail:] == np.float32(0.1)).all(), i
        assert not np.array_equal(g[:-tail], t0[:-tail].astype(np.float32)), i
        move_ref = r[:-tail] - t0[:-tail]
        off = np.linalg.norm((g[:-tail].astype(np.float64) - t0[:-tail]) - move_ref)
        bound = 1e-3 * np.linalg.norm(move_ref) + 1.5 * 2.0 ** -23 * np.linalg.norm(t0[:-tail])
        print("DistMult d=%d k=%d table %d: movement %.3g, off by %.3g (bound %.3g)" % (dim, k, i, np.linalg.norm(move_ref), off, bound))
        assert off <= bound, i
    for t in (s["e"], s["r"]):
        assert float(t[:, dim:].abs().sum()) == 0.0


@pytest.mark.parametrize("k", [1, 10])
def test_distmult_loss_is_the_batch_mean(k):
    """each triple twice leaves a mean unchanged and doubles a sum"""
    from openea_amd import ops
    dev = ops.device()
    rng = np.random.RandomState(5 + k)
    dim = 100
    tables = [_xavier(rng, DM_E, dim), _xavier(rng, DM_R, dim)]
    pos, neg = _zipf_batch(rng, DM_E, DM_R, DM_N, k)
    losses = []
    for p, n in ((pos, neg), (np.concatenate([pos, pos]), np.concatenate([neg, neg]))):
        s = _dm_setup(tables, "Adagrad", dev, k=k)
        _dm_step(s, ops.to_ids(p, dev), ops.to_ids(n, dev))
        losses.append(float(s["loss"].item()))
    print("k=%d: loss %.12g, every triple twice %.12g" % (k, losses[0], losses[1]))
    assert 0.5 < losses[0] < 0.9                                           # softplus(0) = 0.693 per triple at small scores
    assert abs(losses[1] - losses[0]) <= 1e-6 * losses[0]


# ---- 4. the fixed-point build ----------------------------------------------------------------------------------------------------
DET_WORKER = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.environ["OEA_ROOT"]); sys.path.insert(0, os.path.join(os.environ["OEA_ROOT"], "tests"))
import torch
from openea_amd import ops
from test_rotate_distmult_gpu import DM_E, DM_N, DM_R, _dm_setup, _dm_step, _xavier, _zipf_batch
assert ops.deterministic()
dev = ops.device()
runs = []
for _ in range(2):
    rng = np.random.RandomState(7)
    tables = [_xavier(rng, DM_E, 100), _xavier(rng, DM_R, 100)]
    s = _dm_setup(tables, "Adagrad", dev, k=10)
    for _ in range(3):
        pos, neg = _zipf_batch(rng, DM_E, DM_R, DM_N, 10)
        _dm_step(s, ops.to_ids(pos, dev), ops.to_ids(neg, dev))
    torch.cuda.synchronize()
    runs.append((s["e"].cpu().numpy(), s["r"].cpu().numpy(), s["accs"][0].cpu().numpy(), s["accs"][1].cpu().numpy()))
moved = int(not np.array_equal(runs[0][0], ops.to_table(tables[0], dev=dev).cpu().numpy()))
print("RESULT DistMult same_bits=%d moved=%d" % (int(all(np.array_equal(a, b) for a, b in zip(*runs))), moved))
'''


def test_fixed_point_build_gives_the_same_bits():
    """libopenea_hip_det.so (OEA_STEP_DETERMINISTIC=1): int64 fixed-point scratch -- two runs of three DistMult steps give
    bit-identical tables and accumulators"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", DET_WORKER], env=dict(os.environ, OEA_ROOT=root, OEA_STEP_DETERMINISTIC="1"),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "RESULT DistMult same_bits=1 moved=1" in p.stdout, p.stdout


# ---- 5. what the DistMult step refuses -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["model", "Adam", "n_neg", "dim", "ld"])
def test_distmult_rejected_configurations_launch_nothing(bad):
    from openea_amd import ops
    from openea_amd._lib import OpenEAHipError
    dev = ops.device()
    rng = np.random.RandomState(1)
    dim = 129 if bad == "dim" else 30
    s = _dm_setup([rng.randn(50, dim) * 0.1, rng.randn(6, dim) * 0.1], "Adagrad", dev)
    if bad == "ld":                                             # ld = dim = 30, not a multiple of 4
        s["e"] = s["e"][:, :dim].contiguous()
        s["r"] = s["r"][:, :dim].contiguous()
        s["accs"] = [torch.full_like(s["e"], 0.1), torch.full_like(s["r"], 0.1)]
        s["ws"] = ops.step_workspace(50, 6, dim, dev)
    if bad == "Adam":
        s["cfg"] = ops.make_step_cfg(loss="margin-based", optimizer="Adam", lr=0.01, neg_group_k=1)
        s["accs"] = [torch.zeros((2,) + tuple(t.shape), device=dev) for t in (s["e"], s["r"])]
    if bad == "model":
        s["kind"] = 7
    pos = ops.to_ids(np.array([[0, 1, 2], [3, 4, 5]]), dev)
    neg = ops.to_ids(np.array([[0, 1, 7], [9, 4, 5]] + ([[8, 4, 5]] if bad == "n_neg" else [])), dev)
    e0, r0 = s["e"].clone(), s["r"].clone()
    with pytest.raises(OpenEAHipError):
        _dm_step(s, pos, neg)
    torch.cuda.synchronize()
    assert torch.equal(s["e"], e0) and torch.equal(s["r"], r0)
    assert float(s["loss"].item()) == 0.0


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["RotatE", "DistMult"])
def test_end_to_end(name, tmp_path, capsys):
    from openea_amd.models import semantic
    from openea_amd.modules.base import initializers
    from openea_amd.modules.load.synth import make_kgs
    from openea_amd.run.default_args import get_args
    initializers.seed(20190719)
    kgs = make_kgs("small", mode="sharing", seed=0)
    kw = dict(dim=32, batch_size=2000, max_epoch=12, start_valid=4, eval_freq=4)
    if name == "RotatE":
        kw["learning_rate"] = 0.01          # the reference's own header: its shipped 0.1 is NaN-prone at odd shapes
    model = getattr(semantic, name)()
    model.set_args(get_args(name, output=str(tmp_path) + "/out/", training_data="synthetic/small/", dataset_division="fold1/", **kw))
    model.set_kgs(kgs)
    model.init()
    e0, r0 = model.ent_embeds.var.clone(), model.rel_embeds.var.clone()
    before = model.valid("hits1")
    model.run()
    after = model.valid("hits1")
    model.test()
    model.save()
    out = capsys.readouterr().out
    assert "Training ends. Total time" in out and "accurate results: hits@[1, 5, 10, 50]" in out
    if name == "RotatE":
        assert "epoch 12, avg. triple loss: " in out                      # BasicModel's line
    else:
        assert "epoch 12, triple loss: " in out and "avg. triple loss" not in out      # distmult.py:87
    assert after >= before - 1.0
    for t in (model.ent_embeds.var, model.rel_embeds.var):
        assert torch.isfinite(t).all()
    assert not torch.equal(model.ent_embeds.var, e0) and not torch.equal(model.rel_embeds.var, r0)
    E = kgs.entities_num
    ent = np.load(model.out_folder + "ent_embeds.npy")
    assert ent.shape == (E, 32) and ent.dtype == np.float32
    np.testing.assert_allclose(np.linalg.norm(ent, axis=1), 1.0, rtol=1e-5)
    assert np.load(model.out_folder + "rel_embeds.npy").shape == (kgs.relations_num, 32)
    for f in ("kg1_ent_ids", "kg2_ent_ids", "kg1_rel_ids", "alignment_results_12", "kg1_ent_embeds_txt"):
        assert os.path.exists(model.out_folder + f)
    if name == "RotatE":
        assert model.ent_embeds.var.dtype == torch.float64 and model.ent_embeds.var.shape[0] == 2 * E
        assert model._trainer.cfg.neg_loss_div == model._trainer.k == model.args.neg_triple_num == 10
        assert abs(model.embedding_range - 14.0 / 32) < 1e-12
        ids = np.arange(E, dtype=np.int32)
        look = model._lookup(ids)[:, :32].cpu().numpy()
        raw = model.ent_embeds.var[:, :32].cpu().numpy()
        l2n = raw / np.sqrt(np.maximum((raw * raw).sum(1, keepdims=True), 1e-12))
        np.testing.assert_allclose(look, l2n[:E] + l2n[E:], rtol=0, atol=1e-6)
        assert model.re_ent_embeds.shape == model.im_ent_embeds.shape == (E, 32)
        np.testing.assert_allclose(model.re_ent_embeds + model.im_ent_embeds, l2n[:E] + l2n[E:], rtol=0, atol=1e-12)
    else:
        assert model.metric == "inner" and model._trainer.model == 2
