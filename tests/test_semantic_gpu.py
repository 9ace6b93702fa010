"""HolE and SimplE on the device (oea_semantic_step, csrc/semantic_step.hip): against the reference's own graphs
(tests/golden/semantic_graph.npz), against the float64 restatement of test_semantic_cpu.py at the shipped shape, run to run in
the fixed-point build, end to end through the model classes, and the configurations the step refuses."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_semantic_cpu import CASES, GOLDEN, fixture_case, semantic_reference_step  # noqa: E402


def _stack(model, tables):
    """host tables in the device layout: HolE (ent, rel); SimplE ([H; T], [R1; R2])"""
    if model == "HolE":
        return tables[0], tables[1]
    return np.concatenate([tables[0], tables[1]]), np.concatenate([tables[2], tables[3]])


def _unstack(model, ent, rel):
    if model == "HolE":
        return [ent, rel]
    E, R = ent.shape[0] // 2, rel.shape[0] // 2
    return [ent[:E], ent[E:], rel[:R], rel[R:]]


def _setup(model, tables, optimizer, dev, k=1, margin=0.2, lr=0.01):
    from openea_amd import ops
    ent, rel = _stack(model, tables)
    e, r = ops.to_table(ent, dev=dev), ops.to_table(rel, dev=dev)
    cfg = ops.make_step_cfg(loss="margin-based", margin=margin, optimizer=optimizer, lr=lr, neg_group_k=k)
    accs = [torch.full_like(t, 0.1) for t in (e, r)] if optimizer == "Adagrad" else [None, None]
    ws = ops.step_workspace(e.shape[0], r.shape[0], e.shape[1], dev)
    kind = ops.SEMANTIC_HOLE if model == "HolE" else ops.SEMANTIC_SIMPLE
    return dict(kind=kind, model=model, e=e, r=r, accs=accs, cfg=cfg, ws=ws, d=ent.shape[1],
                loss=torch.zeros(1, dtype=torch.float64, device=dev))


def _step(s, pos, neg):
    from openea_amd import ops
    ops.semantic_step(s["kind"], s["e"], s["accs"][0], s["r"], s["accs"][1], s["d"], pos, neg, s["cfg"], s["ws"], s["loss"])


def _host(s, which):
    d = s["d"]
    if which == "tables":
        return _unstack(s["model"], s["e"][:, :d].cpu().numpy(), s["r"][:, :d].cpu().numpy())
    return _unstack(s["model"], s["accs"][0][:, :d].cpu().numpy(), s["accs"][1][:, :d].cpu().numpy())


@pytest.mark.parametrize("case", CASES)
def test_sgd_step_equals_reference_graph(case):
    from openea_amd import ops
    dev = ops.device()
    z = np.load(GOLDEN)
    model, tables, pos, neg, margin, k = fixture_case(z, case)
    lr = 0.01
    s = _setup(model, tables, "SGD", dev, k=k, margin=margin, lr=lr)
    _step(s, ops.to_ids(pos, dev), ops.to_ids(neg, dev))
    loss, ref_loss = float(s["loss"].item()), float(z[case + "_loss"][0])
    assert abs(loss - ref_loss) <= 2e-5 * abs(ref_loss)
    names = ("ent_embeds", "rel_embeds") if model == "HolE" else ("head_ent_embeds", "tail_ent_embeds", "rel_embeds1", "rel_embeds2")
    for name, before, got in zip(names, tables, _host(s, "tables")):
        g = (before.astype(np.float32).astype(np.float64) - got) / lr          # SGD: the update IS lr * gradient
        ref = z["%s_grad_%s" % (case, name)]
        assert np.abs(g - ref).max() <= 1e-3 * np.abs(ref).max(), name


def _zipf_batch(rng, n_ent, n_rel, n, k=1):
    """n positives with Zipf(1.1) relations over the first n_rel - 4 relations (the last 4 appear nowhere), entities from
    [0, n_ent - 100) (the last 100 appear nowhere), one entity in many triples, h == t triples; k corruptions of head or tail
    per positive, some with another relation than their positive's"""
    used = n_ent - 100
    common = n_rel - 4
    p = 1.0 / np.arange(1, common + 1) ** 1.1
    rels = rng.choice(common, n, p=p / p.sum())
    pos = np.stack([rng.randint(0, used, n), rels, rng.randint(0, used, n)], 1).astype(np.int32)
    pos[:20, 0] = pos[0, 0]
    pos[20:30, 2] = pos[20:30, 0]
    neg = np.repeat(pos, k, axis=0)
    side = rng.randint(0, 2, n * k) * 2
    neg[np.arange(n * k), side] = rng.randint(0, used, n * k)
    other = rng.choice(n * k, 50, replace=False)
    neg[other, 1] = rng.randint(0, common, 50)
    return pos, neg


def _xavier(rng, rows, dim):
    from openea_amd.modules.base.initializers import xavier_host
    return xavier_host(rng, (rows, dim)).astype(np.float64)


@pytest.mark.parametrize("model", ["HolE", "SimplE"])
@pytest.mark.parametrize("dim", [8, 75, 100, 128])
def test_adagrad_steps_equal_restatement(model, dim):
    """three Adagrad steps at the EN-FR-15K-V1 batch shape; dim = 75 has ld != dim in the circular index.  Rows no triple
    refers to keep their bits and their accumulators stay at 0.1 (for SimplE in all four halves)."""
    from _tol import assert_rows_close
    from openea_amd import ops
    dev = ops.device()
    rng = np.random.RandomState(dim + (0 if model == "HolE" else 1000))
    n_ent, n_rel, n = 15000, 477, 5000
    n_tab = 1 if model == "HolE" else 2
    tables = [_xavier(rng, n_ent, dim) for _ in range(n_tab)] + [_xavier(rng, n_rel, dim) for _ in range(n_tab)]
    s = _setup(model, tables, "Adagrad", dev)
    ref, accs = [t.copy() for t in tables], [np.full_like(t, 0.1) for t in tables]
    loss_ref = 0.0
    for _ in range(3):
        pos, neg = _zipf_batch(rng, n_ent, n_rel, n)
        loss_ref += semantic_reference_step(model, ref, accs, pos, neg, 0.01, margin=0.2)
        _step(s, ops.to_ids(pos, dev), ops.to_ids(neg, dev))
    loss = float(s["loss"].item())
    assert abs(loss - loss_ref) <= 1e-4 * abs(loss_ref)
    got, got_acc = _host(s, "tables"), _host(s, "accs")
    for i, (g, r) in enumerate(zip(got, ref)):
        assert_rows_close(g, r, "%s d=%d table %d" % (model, dim, i))
    for i, (g, r) in enumerate(zip(got_acc, accs)):
        assert_rows_close(g, r, "%s d=%d accumulator %d" % (model, dim, i))
    for i, (g, a, t0) in enumerate(zip(got, got_acc, tables)):
        tail = 100 if t0.shape[0] == n_ent else 4
        assert np.array_equal(g[-tail:], t0[-tail:].astype(np.float32)), i
        assert (a[-tail:] == np.float32(0.1)).all(), i
        assert not np.array_equal(g[:-tail], t0[:-tail].astype(np.float32)), i


DET_WORKER = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.environ["OEA_ROOT"]); sys.path.insert(0, os.path.join(os.environ["OEA_ROOT"], "tests"))
import torch
from openea_amd import ops
from test_semantic_gpu import _setup, _step, _xavier, _zipf_batch
assert ops.deterministic()
dev = ops.device()
for model in ("HolE", "SimplE"):
    runs = []
    for _ in range(2):
        rng = np.random.RandomState(7)
        n_tab = 1 if model == "HolE" else 2
        tables = [_xavier(rng, 15000, 100) for _ in range(n_tab)] + [_xavier(rng, 477, 100) for _ in range(n_tab)]
        s = _setup(model, tables, "Adagrad", dev)
        for _ in range(3):
            pos, neg = _zipf_batch(rng, 15000, 477, 5000)
            _step(s, ops.to_ids(pos, dev), ops.to_ids(neg, dev))
        torch.cuda.synchronize()
        runs.append((s["e"].cpu().numpy(), s["r"].cpu().numpy(), s["accs"][0].cpu().numpy(), s["accs"][1].cpu().numpy()))
    print("RESULT %s same_bits=%d" % (model, int(all(np.array_equal(a, b) for a, b in zip(*runs)))))
'''


def test_fixed_point_build_gives_the_same_bits():
    """libopenea_hip_det.so (OEA_STEP_DETERMINISTIC=1): int64 fixed-point scratch -- two runs of three steps of each model
    give bit-identical tables and accumulators"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", DET_WORKER], env=dict(os.environ, OEA_ROOT=root, OEA_STEP_DETERMINISTIC="1"),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "RESULT HolE same_bits=1" in p.stdout and "RESULT SimplE same_bits=1" in p.stdout, p.stdout


@pytest.mark.parametrize("bad", ["model", "Adam", "Adadelta", "n_neg", "dim", "ld"])
def test_rejected_configurations_launch_nothing(bad):
    from openea_amd import ops
    from openea_amd._lib import OpenEAHipError
    dev = ops.device()
    rng = np.random.RandomState(1)
    dim = 129 if bad == "dim" else 30
    s = _setup("HolE", [rng.randn(50, dim) * 0.1, rng.randn(6, dim) * 0.1], "Adagrad", dev)
    if bad == "ld":                                             # ld = dim = 30, not a multiple of 4
        s["e"] = s["e"][:, :dim].contiguous()
        s["r"] = s["r"][:, :dim].contiguous()
        s["accs"] = [torch.full_like(s["e"], 0.1), torch.full_like(s["r"], 0.1)]
        s["ws"] = ops.step_workspace(50, 6, dim, dev)
    if bad in ("Adam", "Adadelta"):
        s["cfg"] = ops.make_step_cfg(loss="margin-based", margin=0.2, optimizer=bad, lr=0.01, neg_group_k=1)
        s["accs"] = [torch.zeros((2,) + tuple(t.shape), device=dev) for t in (s["e"], s["r"])]
    if bad == "model":
        s["kind"] = 7
    pos = ops.to_ids(np.array([[0, 1, 2], [3, 4, 5]]), dev)
    neg = ops.to_ids(np.array([[0, 1, 7], [9, 4, 5]] + ([[8, 4, 5]] if bad == "n_neg" else [])), dev)
    e0, r0 = s["e"].clone(), s["r"].clone()
    with pytest.raises(OpenEAHipError):
        _step(s, pos, neg)
    torch.cuda.synchronize()
    assert torch.equal(s["e"], e0) and torch.equal(s["r"], r0)
    assert float(s["loss"].item()) == 0.0


@pytest.mark.parametrize("name", ["HolE", "SimplE"])
def test_end_to_end(name, tmp_path, capsys):
    from openea_amd import ops
    from openea_amd.models import semantic
    from openea_amd.modules.base import initializers
    from openea_amd.modules.load.synth import make_kgs
    from openea_amd.run.default_args import get_args
    initializers.seed(20190719)
    kgs = make_kgs("small", mode="sharing", seed=0)
    kw = dict(dim=32, batch_size=2000, max_epoch=12, start_valid=4, eval_freq=4)
    model = getattr(semantic, name)()
    model.set_args(get_args(name, output=str(tmp_path) + "/out/", training_data="synthetic/small/", dataset_division="fold1/", **kw))
    model.set_kgs(kgs)
    model.init()
    e0 = model.ent_embeds.var.clone()
    before = model.valid("hits1")
    model.run()
    after = model.valid("hits1")
    model.test()
    model.save()
    out = capsys.readouterr().out
    assert "Training ends. Total time" in out and "accurate results: hits@[1, 5, 10, 50]" in out
    assert "avg. triple loss" in out
    assert after >= before - 1.0
    for t in (model.ent_embeds.var, model.rel_embeds.var):
        assert torch.isfinite(t).all()
    assert not torch.equal(model.ent_embeds.var, e0)
    ent = np.load(model.out_folder + "ent_embeds.npy")
    assert ent.shape == (kgs.entities_num, 32) and ent.dtype == np.float32
    assert np.load(model.out_folder + "rel_embeds.npy").shape == (kgs.relations_num, 32)
    for f in ("kg1_ent_ids", "kg2_ent_ids", "kg1_rel_ids", "alignment_results_12", "kg1_ent_embeds_txt"):
        assert os.path.exists(model.out_folder + f)
    if name == "SimplE":
        np.testing.assert_allclose(np.linalg.norm(ent, axis=1), 1.0, rtol=1e-5)
        ids = np.arange(kgs.entities_num, dtype=np.int32)
        look = model._lookup(ids)[:, :32].cpu().numpy()
        np.testing.assert_allclose(look, model.head_ent_embeds + model.tail_ent_embeds, rtol=0, atol=1e-6)
        raw = model.ent_embeds.var[:, :32].cpu().numpy().astype(np.float64)
        l2n = raw / np.maximum(np.linalg.norm(raw, axis=1, keepdims=True), 1e-6)
        E = kgs.entities_num
        np.testing.assert_allclose(look, l2n[:E] + l2n[E:], rtol=0, atol=1e-5)
        assert model.rel_embeds1.shape == model.rel_embeds2.shape == (kgs.relations_num, 32)
    else:
        np.testing.assert_allclose(np.linalg.norm(ent, axis=1), 1.0, rtol=1e-5)
    assert ops.SEMANTIC_MAX_DIM == 128
