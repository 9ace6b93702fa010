"""TransR on the device (oea_transr_step, csrc/transr_step.hip): against the reference's own graph
(tests/golden/transr_graph.npz), against the float64 restatement of test_transr_cpu.py at the shipped shape, run to run, end
to end through the model class, and the configurations it refuses."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_transr_cpu import GOLDEN, transr_reference_step  # noqa: E402


def _setup(ent, rel, mat, optimizer, dev, **cfg_kw):
    from openea_amd import ops
    d = ent.shape[1]
    e, r = ops.to_table(ent, dev=dev), ops.to_table(rel, dev=dev)
    m = torch.from_numpy(np.ascontiguousarray(mat, np.float32)).to(dev)
    kw = dict(loss="margin-based", loss_norm="L2", margin=1.5, optimizer=optimizer, lr=0.01)
    kw.update(cfg_kw)
    cfg = ops.make_step_cfg(**kw)
    accs = [torch.full_like(t, 0.1) for t in (e, r, m)] if optimizer == "Adagrad" else [None] * 3
    ws = ops.step_workspace(e.shape[0], r.shape[0], e.shape[1], dev)
    return dict(e=e, r=r, m=m, accs=accs, cfg=cfg, ws=ws, d=d, loss=torch.zeros(1, dtype=torch.float64, device=dev))


def _step(s, pos, neg, tws=None):
    from openea_amd import ops
    if tws is None:
        tws = ops.transr_workspace(s["e"].shape[0], s["r"].shape[0], s["d"], pos.shape[0], s["e"].device)
    ops.transr_step(s["e"], s["accs"][0], s["r"], s["accs"][1], s["m"], s["accs"][2], s["d"], pos, neg, s["cfg"], s["ws"], tws,
                    s["loss"])
    return tws


@pytest.mark.parametrize("case", ["tiny", "d16"])
def test_sgd_step_equals_reference_graph(case):
    from openea_amd import ops
    dev = ops.device()
    z = np.load(GOLDEN)
    ent, rel, mat = (z["%s_var_%s" % (case, n)] for n in ("ent_embeds", "rel_embeds", "rel_matrix"))
    lr = 0.01
    s = _setup(ent, rel, mat, "SGD", dev, margin=float(z[case + "_margin"][0]), lr=lr)
    d = s["d"]
    _step(s, ops.to_ids(z[case + "_pos"], dev), ops.to_ids(z[case + "_neg"], dev))
    loss = float(s["loss"].item())
    ref_loss = float(z[case + "_loss"][0])
    assert abs(loss - ref_loss) <= 2e-5 * abs(ref_loss)
    got = {"ent_embeds": s["e"][:, :d].cpu().numpy(), "rel_embeds": s["r"][:, :d].cpu().numpy(), "rel_matrix": s["m"].cpu().numpy()}
    before = {"ent_embeds": ent, "rel_embeds": rel, "rel_matrix": mat}
    for name in got:
        g = (before[name].astype(np.float32).astype(np.float64) - got[name]) / lr     # SGD: the update IS lr * gradient
        ref = z["%s_grad_%s" % (case, name)]
        assert np.abs(g - ref).max() <= 1e-3 * np.abs(ref).max(), name


def _zipf_batch(rng, n_ent, n_rel, n, dim):
    """n pairs with Zipf(1.1) relations over the first n_rel - 12 relations, 8 relations that appear exactly once (a one-pair
    tile), 4 that do not appear at all; duplicate entities; some negatives with another relation than their positive's"""
    common = n_rel - 12
    p = 1.0 / np.arange(1, common + 1) ** 1.1
    rels = rng.choice(common, n, p=p / p.sum())
    rels[-8:] = np.arange(common, common + 8)
    pos = np.stack([rng.randint(0, n_ent, n), rels, rng.randint(0, n_ent, n)], 1).astype(np.int32)
    neg = pos.copy()
    side = rng.randint(0, 2, n) * 2
    neg[np.arange(n), side] = rng.randint(0, n_ent, n)
    other = rng.choice(n - 8, 50, replace=False)
    neg[other, 1] = rng.randint(0, common, 50)
    pos[:20, 0] = pos[0, 0]                                        # one entity in many triples
    return pos, neg


@pytest.mark.parametrize("dim", [8, 75, 100, 128])
def test_adagrad_steps_equal_restatement(dim):
    from _tol import assert_rows_close
    from openea_amd import ops
    from openea_amd.modules.base.initializers import truncated_normal_host
    dev = ops.device()
    rng = np.random.RandomState(dim)
    n_ent, n_rel, n = 15000, 477, 5000
    ent = truncated_normal_host(rng, (n_ent, dim), 1.0 / np.sqrt(dim)).astype(np.float64)
    rel = truncated_normal_host(rng, (n_rel, dim), 1.0 / np.sqrt(dim)).astype(np.float64)
    mat = truncated_normal_host(rng, (n_rel, dim * dim), 1.0 / dim).astype(np.float64)
    s = _setup(ent, rel, mat, "Adagrad", dev)
    tables, accs = [ent.copy(), rel.copy(), mat.copy()], [np.full_like(ent, 0.1), np.full_like(rel, 0.1), np.full_like(mat, 0.1)]
    batches = [_zipf_batch(rng, n_ent, n_rel, n, dim) for _ in range(3)]
    counts = np.bincount(np.concatenate([batches[0][0][:, 1], batches[0][1][:, 1]]), minlength=n_rel)
    assert counts.max() * 2 > 1000 and (counts[-12:-4] == 2).all() and (counts[-4:] == 0).all()   # one pair each: a 2-item tile
    loss_ref = 0.0
    tws = None
    for pos, neg in batches:
        loss_ref += transr_reference_step(tables, accs, pos, neg, 1.5, 0.01)
        tws = _step(s, ops.to_ids(pos, dev), ops.to_ids(neg, dev), tws)
    loss = float(s["loss"].item())
    assert abs(loss - loss_ref) <= 1e-4 * abs(loss_ref)
    got = [s["e"][:, :dim].cpu().numpy(), s["r"][:, :dim].cpu().numpy(), s["m"].cpu().numpy()]
    got_acc = [s["accs"][0][:, :dim].cpu().numpy(), s["accs"][1][:, :dim].cpu().numpy(), s["accs"][2].cpu().numpy()]
    for name, g, ref in zip(("ent", "rel", "rel_matrix"), got, tables):
        assert_rows_close(g, ref, "TransR d=%d %s" % (dim, name))
    for name, g, ref in zip(("ent_acc", "rel_acc", "rel_matrix_acc"), got_acc, accs):
        assert_rows_close(g, ref, "TransR d=%d %s" % (dim, name))
    # the four relations no batch refers to: bit-identical matrix and accumulator
    assert np.array_equal(got[2][-4:], mat[-4:].astype(np.float32))
    assert (got_acc[2][-4:] == np.float32(0.1)).all()


def test_one_step_is_reproducible():
    from openea_amd import ops
    from openea_amd.modules.base.initializers import truncated_normal_host
    dev = ops.device()
    rng = np.random.RandomState(5)
    n_ent, n_rel, n, dim = 15000, 477, 5000, 100
    ent = truncated_normal_host(rng, (n_ent, dim), 0.1)
    rel = truncated_normal_host(rng, (n_rel, dim), 0.1)
    mat = truncated_normal_host(rng, (n_rel, dim * dim), 0.01)
    pos, neg = _zipf_batch(rng, n_ent, n_rel, n, dim)
    out = []
    for _ in range(2):
        s = _setup(ent, rel, mat, "Adagrad", dev)
        _step(s, ops.to_ids(pos, dev), ops.to_ids(neg, dev))
        out.append((s["m"].cpu().numpy(), s["accs"][2].cpu().numpy()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert not np.array_equal(out[0][0], mat.astype(np.float32))


@pytest.mark.parametrize("bad", [dict(dim=129), dict(loss_norm="L1"), dict(loss="limited", pos_margin=0.01, neg_margin=2.0),
                                 dict(optimizer="Adam")])
def test_rejected_configurations_launch_nothing(bad):
    from openea_amd import ops
    from openea_amd._lib import OpenEAHipError
    dev = ops.device()
    rng = np.random.RandomState(1)
    dim = bad.pop("dim", 32)
    ent, rel = rng.randn(50, dim) * 0.1, rng.randn(6, dim) * 0.1
    mat = rng.randn(6, dim * dim) * 0.1
    opt = bad.pop("optimizer", "Adagrad")
    s = _setup(ent, rel, mat, opt, dev, **bad)
    if opt == "Adam":
        s["accs"] = [torch.zeros((2,) + tuple(t.shape), device=dev) for t in (s["e"], s["r"], s["m"])]
    pos = ops.to_ids(np.array([[0, 1, 2], [3, 4, 5]]), dev)
    neg = ops.to_ids(np.array([[0, 1, 7], [9, 4, 5]]), dev)
    e0, r0, m0 = s["e"].clone(), s["r"].clone(), s["m"].clone()
    with pytest.raises(OpenEAHipError):
        _step(s, pos, neg)
    torch.cuda.synchronize()
    assert torch.equal(s["e"], e0) and torch.equal(s["r"], r0) and torch.equal(s["m"], m0)
    assert float(s["loss"].item()) == 0.0


def test_transr_end_to_end(tmp_path, capsys):
    from openea_amd.models.trans import TransR
    from openea_amd.modules.base import initializers
    from openea_amd.modules.load.synth import make_kgs
    from openea_amd.run.default_args import get_args
    initializers.seed(20190719)
    kgs = make_kgs("small", mode="sharing", seed=0)
    kw = dict(dim=32, batch_size=2000, max_epoch=12, start_valid=4, eval_freq=4)
    model = TransR()
    model.set_args(get_args("TransR", output=str(tmp_path) + "/out/", training_data="synthetic/small/", dataset_division="fold1/", **kw))
    model.set_kgs(kgs)
    model.init()
    m0 = model.rel_matrix.copy()
    before = model.valid("hits1")
    model.run()
    after = model.valid("hits1")
    model.test()
    model.save()
    out = capsys.readouterr().out
    assert "Training ends. Total time" in out and "accurate results: hits@[1, 5, 10, 50]" in out
    assert after >= before - 1.0
    ent = np.load(model.out_folder + "ent_embeds.npy")
    assert ent.shape == (kgs.entities_num, 32) and ent.dtype == np.float32
    np.testing.assert_allclose(np.linalg.norm(ent, axis=1), 1.0, rtol=1e-5)
    assert np.load(model.out_folder + "rel_embeds.npy").shape == (kgs.relations_num, 32)
    for f in ("kg1_ent_ids", "kg2_ent_ids", "kg1_rel_ids", "alignment_results_12", "kg1_ent_embeds_txt"):
        assert os.path.exists(model.out_folder + f)
    assert model.rel_matrix.shape == (kgs.relations_num, 32 * 32)
    assert not np.array_equal(model.rel_matrix, m0) and np.isfinite(model.rel_matrix).all()
