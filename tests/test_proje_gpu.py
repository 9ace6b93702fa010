"""ProjE on the device (csrc/proje_step.hip): the log-uniform sampler (csrc/log_uniform.hip) against its numpy restatement, the gradient phase of
oea_proje_step against the reference's own graph (tests/golden/proje_graph.npz) and against the float64 restatement of
test_proje_cpu.py at the shapes that have tails, three Adam steps at the EN-FR-15K-V1 batch shape, run to run in the fixed-point
build, the configurations the step refuses, and the model class end to end."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_proje_cpu import (CASES, GOLDEN, VARS, ZERO_GRADS, fixture_case, log_q, log_uniform_reference, make_variables,  # noqa: E402
                            proje_loss_and_grads, proje_reference_step, zipf_batch)

U32 = 2.0 ** -24          # unit roundoff of fp32


# ---- the sampler -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_classes,n_sampled", [(300, 64), (97, 97), (1000, 257), (27000, 4096), (180000, 4096)])
def test_sampler_equals_restatement(n_classes, n_sampled):
    from openea_amd import ops
    dev = ops.device()
    for seed, step in ((11, 0), (2 ** 40 + 5, 3)):
        s = ops.LogUniformSampler(n_classes, n_sampled, seed, dev)
        ids, tries, lq = (x.clone() for x in s.sample(step))
        ref_ids, ref_tries, ref_lq = log_uniform_reference(n_classes, n_sampled, seed, step)
        assert np.array_equal(ids.cpu().numpy(), ref_ids)
        assert int(tries.item()) == ref_tries
        err = np.abs(lq.cpu().numpy().astype(np.float64) - ref_lq).max()
        print("E %d S %d: num_tries %d, max |log Q - fp64| %.3g" % (n_classes, n_sampled, ref_tries, err))
        assert err <= 1e-6
        ids2, tries2, lq2 = s.sample(step)                    # the workspace was left clean: the same bits again
        assert torch.equal(ids, ids2) and torch.equal(tries, tries2) and torch.equal(lq.view(torch.int32), lq2.view(torch.int32))
        assert int(s.workspace.view(torch.int32)[:n_classes].abs().max().item()) == 0


@pytest.mark.parametrize("bad", ["S>E", "null table"])
def test_sampler_refusals_leave_the_outputs(bad):
    from openea_amd import ops
    from openea_amd._lib import OpenEAHipError
    dev = ops.device()
    s = ops.LogUniformSampler(50, 60 if bad == "S>E" else 20, 3, dev)
    s.ids.fill_(-7)
    s.num_tries.fill_(-7)
    s.log_q.fill_(-7.0)
    if bad == "null table":
        s.thresholds = None
    with pytest.raises(OpenEAHipError):
        s.sample(0)
    torch.cuda.synchronize()
    assert (s.ids == -7).all() and (s.num_tries == -7).all() and (s.log_q == -7.0).all()


# ---- the step ----------------------------------------------------------------------------------------------------------------
def _setup(variables, max_pos, max_s, dev):
    """host variables (order VARS, tables [n, d]) -> device state"""
    from openea_amd import ops
    d = variables[0].shape[1]
    dv = [ops.to_table(v, dev=dev) if v.ndim == 2 else ops.to_vec(v, dev) for v in variables]
    ws = ops.proje_workspace(dv[0].shape[0], dv[1].shape[0], d, dv[0].shape[1], max_pos, max_s, dev)
    return dict(v=dv, m=[torch.zeros_like(x) for x in dv], w=[torch.zeros_like(x) for x in dv], ws=ws, d=d,
                loss=torch.zeros(1, dtype=torch.float64, device=dev))


def _step(s, pos, sampled, num_tries, log_q_dev=None, t=1, lr=0.001, phase=None):
    from openea_amd import ops
    dev = s["v"][0].device
    n_ent = s["v"][0].shape[0]
    if not hasattr(sampled, "is_cuda"):
        log_q_dev = ops.to_vec(log_q(sampled, num_tries, n_ent), dev)
        sampled = ops.to_ids(sampled, dev)
        num_tries = torch.tensor([num_tries], dtype=torch.int64, device=dev)
    ops.proje_step(s["v"], s["m"], s["w"], s["d"], ops.to_ids(pos, dev), sampled, log_q_dev, num_tries, t, lr, s["ws"], s["loss"],
                   phase=ops.PHASE_BOTH if phase is None else phase)


def _host(tensors, d):
    return [x[:, :d].cpu().numpy() if x.dim() == 2 else x.cpu().numpy() for x in tensors]


def _check_grad_phase(variables, pos, sampled, num_tries, ref_loss, ref_grads, scale, what):
    """loss within 2e-5 relative, every gradient within 1e-3 max|ref|.  The two gradients that are zero identically (the input
    beta and mlp_bias: test_proje_cpu.proje_loss_and_grads) are sums over the batch whose terms cancel; what fp32 leaves of them
    is bounded by a handful (8) of roundings of each term, 8 * 2^-24 * scale, on top of the relative bound."""
    from openea_amd import ops
    dev = ops.device()
    s = _setup(variables, len(pos), len(sampled), dev)
    before = [x.clone() for x in s["v"]]
    _step(s, pos, sampled, num_tries, phase=ops.PHASE_GRAD)
    loss = float(s["loss"].item())
    print("%s: loss %.9g (reference %.9g, relative %.3g)" % (what, loss, ref_loss, abs(loss - ref_loss) / abs(ref_loss)))
    grads = _host(ops.proje_grads(s["ws"]), s["d"])
    worst = []
    for i, (name, g, ref) in enumerate(zip(VARS, grads, ref_grads)):
        tol = 1e-3 * np.abs(ref).max() + (8 * U32 * scale[i] if i in ZERO_GRADS else 0.0)
        err = np.abs(g - ref).max()
        print("  %-15s max |g - ref| %.3g  (tolerance %.3g, max |ref| %.3g)" % (name, err, tol, np.abs(ref).max()))
        worst.append((name, err, tol))
    assert abs(loss - ref_loss) <= 2e-5 * abs(ref_loss)
    for name, err, tol in worst:
        assert err <= tol, name
    assert all(torch.equal(a, b) for a, b in zip(before, s["v"])), "the gradient phase moved a variable"
    return s, grads


@pytest.mark.parametrize("case", CASES)
def test_gradient_phase_equals_reference_graph(case):
    z = np.load(GOLDEN)
    variables, pos, sampled, num_tries = fixture_case(z, case)
    _, _, scale = proje_loss_and_grads(variables, pos, sampled, num_tries, with_scale=True)
    ref = [z["%s_grad_%s" % (case, n)] for n in VARS]
    _check_grad_phase(variables, pos, sampled, num_tries, float(z[case + "_loss"][0]), ref, scale, case)


@pytest.mark.parametrize("B,S,d", [(3, 2, 8), (33, 97, 75), (70, 200, 100), (130, 257, 128)])
def test_gradient_phase_at_the_edge_shapes(B, S, d):
    """a batch tail against the 32-row tile, a candidate tail, an odd d with ld != d, d at the limit, S below one tile"""
    from openea_amd import ops
    n_ent, n_rel = 400, 12
    rng = np.random.RandomState(1000 * B + d)
    variables = make_variables(rng, n_ent, n_rel, d)
    sampled, num_tries, _ = log_uniform_reference(n_ent, S, 17, B)
    pos = zipf_batch(rng, n_ent, n_rel, B, sampled)
    loss, ref, scale = proje_loss_and_grads(variables, pos, sampled, num_tries, with_scale=True)
    s, grads = _check_grad_phase(variables, pos, sampled, num_tries, float(loss), ref, scale, "B %d S %d d %d" % (B, S, d))
    # rows nothing referred to: exactly zero, pad columns included
    full = [x.cpu().numpy() for x in ops.proje_grads(s["ws"])]
    assert not full[0][-50:].any() and not full[1][-2:].any()
    unused = np.setdiff1d(np.arange(n_ent), np.concatenate([pos[:, 2], sampled]))
    assert len(unused) and not full[2][unused].any() and not full[3][unused].any()
    assert full[2][sampled].any() and full[0][pos[:, 0]].any()
    # a second gradient phase with another batch leaves no row of the first behind
    pos2 = pos.copy()
    pos2[:, 0] = (pos2[:, 0] + 1) % (n_ent - 50)
    _step(s, pos2, sampled, num_tries, phase=ops.PHASE_GRAD)
    _, ref2 = proje_loss_and_grads(variables, pos2, sampled, num_tries)
    g2 = _host(ops.proje_grads(s["ws"]), d)
    assert np.abs(g2[0] - ref2[0]).max() <= 1e-3 * np.abs(ref2[0]).max()


# the restatement's own fp32 noise after three Adam steps, measured on the CPU: the float64 restatement against the same
# restatement with every array held in float32, same inputs, per-row deviation as _tol.assert_rows_close measures it
# (vectors as one row).  In its first steps Adam divides a gradient by its own magnitude, so an element whose gradient is
# near zero moves by up to lr per step on rounding noise alone -- for the input beta and mlp_bias (gradient zero identically)
# that is every element.  Order: VARS.
FP32_NOISE = {
    75: (2.63e-3, 4.16e-5, 4.37e-3, 2.46e-8, 1.36e-2, 7.48e-8, 1.39e-2, 2.47e-7),
    100: (2.63e-3, 9.56e-5, 2.61e-3, 2.41e-8, 1.73e-2, 1.22e-7, 1.73e-2, 6.62e-7),
}


def adam_tolerances(dim):
    """4 x the measured noise (the margin covers another summation order); the project's 1e-4 where it is below 2.5e-5"""
    return [4 * x if x >= 2.5e-5 else 1e-4 for x in FP32_NOISE[dim]]


def _adam_run(dim, dev, reference=True, seed=5):
    """three steps at the 15K batch shape, the sampler stepped on the device -> (state, restatement state, losses)"""
    from openea_amd import ops
    n_ent, n_rel, B, S, lr = 27000, 477, 500, 4096, 0.001
    rng = np.random.RandomState(dim)
    variables = make_variables(rng, n_ent, n_rel, dim)
    s = _setup(variables, B, S, dev)
    sampler = ops.LogUniformSampler(n_ent, S, seed, dev)
    ref = dict(v=[x.copy() for x in variables], m=[np.zeros_like(x) for x in variables], w=[np.zeros_like(x) for x in variables])
    losses, touched = [], dict(h=[], r=[], w=[])
    for step in range(3):
        ids, tries, lq = sampler.sample(step)
        ids_h, tries_h = ids.cpu().numpy().astype(np.int64), int(tries.item())
        pos = zipf_batch(rng, n_ent, n_rel, B, ids_h)
        s["loss"].zero_()
        _step(s, pos, ids, tries, lq, t=step + 1, lr=lr)
        got = float(s["loss"].item())
        want = proje_reference_step(ref["v"], ref["m"], ref["w"], pos, ids_h, tries_h, step + 1, lr) if reference else got
        losses.append((got, want))
        touched["h"].append(pos[:, 0]); touched["r"].append(pos[:, 1]); touched["w"].append(np.concatenate([pos[:, 2], ids_h]))
    return s, ref, losses, variables, {k: np.unique(np.concatenate(v)) for k, v in touched.items()}


@pytest.mark.parametrize("dim", [75, 100])
def test_adam_steps_equal_restatement(dim):
    """Three Adam steps, E = 27,000, R = 477, B = 500, S = 4,096, device state carried across the steps.  Loss of each step within
    1e-4 relative of the restatement fed the same sampled ids.  Variables: per-row deviation within 4 x the restatement's own fp32
    noise (FP32_NOISE, measured on the CPU: d = 75: ent 2.63e-3, rel 4.16e-5, entity_w 4.37e-3, input beta 1.36e-2, mlp_bias
    1.39e-2; d = 100: 2.63e-3, 9.56e-5, 2.61e-3, 1.73e-2, 1.73e-2; entity_b, mlp_w and the output beta below 2.5e-5 -> 1e-4).

    Measured on an MI355X: d = 75: ent_embeds 2.4e-6, rel_embeds 2.7e-6, entity_w 1.2e-4; d = 100: 7.9e-8, 7.5e-7, 1.5e-6; the two
    zero-gradient vectors 1.1e-2 - 1.7e-2."""
    from _tol import assert_rows_close
    from openea_amd import ops
    dev = ops.device()
    s, ref, losses, start, touched = _adam_run(dim, dev)
    for got, want in losses:
        print("loss %.9g restatement %.9g relative %.3g" % (got, want, abs(got - want) / abs(want)))
    for got, want in losses:
        assert abs(got - want) <= 1e-4 * abs(want)
    got_v = _host(s["v"], dim)
    worst = []
    for name, g, r, tol in zip(VARS, got_v, ref["v"], adam_tolerances(dim)):
        g, r = (g, r) if g.ndim == 2 else (g[None], r[None])
        worst.append((name, assert_rows_close(g, r, "d=%d %s (tolerance %.3g)" % (dim, name, tol), tol=np.inf)[0], tol))
    # rows nothing referred to keep their bits, their moments stay 0
    n_ent, n_rel = start[0].shape[0], start[1].shape[0]
    for i, key, n in ((0, "h", n_ent), (1, "r", n_rel), (2, "w", n_ent), (3, "w", n_ent)):
        rest = np.setdiff1d(np.arange(n), touched[key])
        assert len(rest) > 0
        assert np.array_equal(got_v[i][rest], start[i][rest].astype(np.float32)), VARS[i]
        assert not s["m"][i].cpu().numpy()[rest].any() and not s["w"][i].cpu().numpy()[rest].any(), VARS[i]
        assert not np.array_equal(got_v[i][touched[key]], start[i][touched[key]].astype(np.float32)), VARS[i]
    for name, dev_, tol in worst:
        assert dev_ <= tol, "d=%d %s: row deviation %.3g > %.3g" % (dim, name, dev_, tol)


DET_WORKER = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.environ["OEA_ROOT"]); sys.path.insert(0, os.path.join(os.environ["OEA_ROOT"], "tests"))
import torch
from openea_amd import ops
from test_proje_gpu import _adam_run
assert ops.deterministic()
dev = ops.device()
runs = []
for _ in range(2):
    s = _adam_run(100, dev, reference=False)[0]
    torch.cuda.synchronize()
    runs.append([x.cpu().numpy() for x in s["v"] + s["m"] + s["w"]])
print("RESULT same_bits=%d arrays=%d" % (int(all(np.array_equal(a, b) for a, b in zip(*runs))), len(runs[0])))
'''


def test_fixed_point_build_gives_the_same_bits():
    """libopenea_hip_det.so (OEA_STEP_DETERMINISTIC=1): two runs of three steps give bit-identical variables and moments"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", DET_WORKER], env=dict(os.environ, OEA_ROOT=root, OEA_STEP_DETERMINISTIC="1"),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "RESULT same_bits=1 arrays=24" in p.stdout, p.stdout


@pytest.mark.parametrize("bad", ["dim", "ld", "S", "label"])
def test_refusals_launch_nothing(bad):
    from openea_amd import ops
    from openea_amd._lib import OpenEAHipError
    dev = ops.device()
    rng = np.random.RandomState(2)
    n_ent, n_rel, d = 60, 6, 30
    variables = make_variables(rng, n_ent, n_rel, d)
    s = _setup(variables, 4, 8, dev)
    sampled = np.array([3, 9, 1, 20, 7, 11, 0, 5])
    pos = np.array([[0, 1, 2], [3, 4, 5], [0, 2, 9], [8, 1, 8]])
    shape = list(s["ws"]._proje_shape)
    if bad == "dim":                                  # d = 132 in tables of ld = 132
        wide = make_variables(rng, n_ent, n_rel, 132)
        s["v"] = [ops.to_table(v, dev=dev) if v.ndim == 2 else ops.to_vec(v, dev) for v in wide]
        s["m"], s["w"], s["d"] = [torch.zeros_like(x) for x in s["v"]], [torch.zeros_like(x) for x in s["v"]], 132
        shape[2], shape[3] = 132, 132
    if bad == "ld":                                   # ld = dim = 30, not a multiple of 4
        s["v"] = [x[:, :d].contiguous() if x.dim() == 2 else x for x in s["v"]]
        s["m"], s["w"] = [torch.zeros_like(x) for x in s["v"]], [torch.zeros_like(x) for x in s["v"]]
        shape[3] = d
    if bad == "S":
        sampled = sampled[:1]
    if bad == "label":
        pos[2, 2] = n_ent
    s["ws"]._proje_shape = tuple(shape)
    before = [x.clone() for x in s["v"]]
    with pytest.raises(OpenEAHipError) as e:
        _step(s, pos, sampled, 9)
    torch.cuda.synchronize()
    print(bad, "->", e.value)
    assert {"dim": "error -4", "ld": "error -1", "S": "error -1", "label": "outside its table"}[bad] in str(e.value)
    assert all(torch.equal(a, b) for a, b in zip(before, s["v"]))
    assert all(not x.any() for x in s["m"] + s["w"]) and float(s["loss"].item()) == 0.0 and not s["ws"].any()


def test_end_to_end(tmp_path, capsys):
    """learning_rate 0.01: at the shipped 0.001 three epochs of 14 steps are too few for the loss to come down -- the float64
    restatement's own epoch losses on this KG are 128.85, 128.96, 132.16 (they fall at 0.01: 126.99, 111.51, 87.44)"""
    from openea_amd.models.neural import ProjE
    from openea_amd.modules.base import initializers
    from openea_amd.modules.load.synth import make_kgs
    from openea_amd.run.default_args import get_args
    initializers.seed(20190719)
    kgs = make_kgs("tiny", mode="sharing", seed=0)
    model = ProjE()
    model.set_args(get_args("ProjE", output=str(tmp_path) + "/out/", training_data="synthetic/tiny/", dataset_division="fold1/",
                            dim=32, dnn_neg_nums=64, batch_size=200, max_epoch=3, start_valid=3, eval_freq=1, learning_rate=0.01))
    model.set_kgs(kgs)
    model.init()
    e0, w0 = model.ent_embeds.var.clone(), model.entity_w.var.clone()
    model.run()
    model.valid("hits1")
    model.test()
    model.save()
    out = capsys.readouterr().out
    assert "Training ends. Total time" in out and "accurate results: hits@[1, 5, 10, 50]" in out
    losses = [float(x) for x in re.findall(r"epoch \d+, avg\. triple loss: ([-0-9.naninf]+),", out)]
    print(losses)
    assert len(losses) == 3 and np.isfinite(losses).all() and losses[2] < losses[0]
    for t in model.variables():
        assert torch.isfinite(t).all()
    assert not torch.equal(model.ent_embeds.var, e0) and not torch.equal(model.entity_w.var, w0)
    ent = np.load(model.out_folder + "ent_embeds.npy")
    assert ent.shape == (kgs.entities_num, 32) and ent.dtype == np.float32
    np.testing.assert_allclose(np.linalg.norm(ent, axis=1), 1.0, rtol=1e-5)
    for name in ("ent_embeds", "rel_embeds", "entity_w", "entity_b", "triple_loss", "triple_optimizer"):
        assert getattr(model, name) is not None
