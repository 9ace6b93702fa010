"""SEA on the device (oea_sea_mapping_step / oea_sea_mapping_epoch, csrc/sea_mapping.hip): against the reference's own graph
(tests/golden/sea_graph.npz), against the float64 restatement of test_sea_cpu.py at the shipped shapes, run to run, the epoch call
against the step loop, the configurations the step refuses, and end to end through the SEA class."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_sea_cpu import CASES, GOLDEN, fixture_case, sea_reference_step  # noqa: E402

# Adam's m / (sqrt(v) + eps) is ill-conditioned where the true gradient element is within fp32 rounding of zero.  The gradient
# of an entity element is a sum of terms of size up to ~0.05 (2 alpha_1 |x_c| / |P|_F and the products with M^T), so fp32 carries
# it with an absolute error of a few 6e-8 * 0.05 = 3e-9; a quotient good to 1e-2 (1e-4 of a row after lr = 0.01) needs
# |g| >= 100 * 3e-9.  Elements whose float64 gradient stays under TAU in all three steps are left out of the row comparison.
TAU = 3e-7
MASK_CAP = 1e-3


def _setup(ent, rel, m1, m2, optimizer, dev, lr=0.01):
    from openea_amd import ops
    e, r = ops.to_table(ent, dev=dev), ops.to_table(rel, dev=dev)
    d = np.asarray(ent).shape[1]
    adam = optimizer in ("Adam", "Adadelta")
    return dict(e=e, r=r, d=d, opt=optimizer, cfg=ops.make_step_cfg(loss="positive", optimizer=optimizer, lr=lr),
                e_acc=torch.zeros((2,) + tuple(e.shape), device=dev) if adam else None,
                r_acc=torch.zeros((2,) + tuple(r.shape), device=dev) if adam else None,
                m1=torch.from_numpy(np.asarray(m1, np.float32)).to(dev).contiguous(),
                m2=torch.from_numpy(np.asarray(m2, np.float32)).to(dev).contiguous(),
                mst=torch.zeros((4, d, d), device=dev) if adam else None,
                ws=ops.step_workspace(e.shape[0], r.shape[0], e.shape[1], dev), t=0, work=None,
                loss=torch.zeros(1, dtype=torch.float64, device=dev), step_loss=torch.zeros(1, dtype=torch.float64, device=dev),
                empty=torch.zeros((0, 3), dtype=torch.int32, device=dev))


def _step(s, batches, alpha=(2.5, 0.25)):
    """the mapping step + the apply phase of the step engine under the same cfg"""
    from openea_amd import ops
    dev = s["e"].device
    ids = [ops.to_ids(np.asarray(b, np.int32), dev) for b in batches]
    s["t"] += 1
    s["cfg"].opt_t = s["t"]
    s["work"] = ops.sea_mapping_step(s["e"], s["d"], ids[0], ids[1], ids[2], ids[3], s["m1"], s["m2"], s["mst"], alpha[0], alpha[1],
                                     s["cfg"], s["ws"], s["e"].shape[0], s["r"].shape[0], s["loss"], s["work"])
    ops.triple_step(s["e"], s["e_acc"], s["r"], s["r_acc"], s["d"], s["empty"], None, s["cfg"], s["ws"], s["step_loss"],
                    phase=ops.PHASE_APPLY)


@pytest.mark.parametrize("case", CASES)
def test_sgd_step_equals_reference_graph(case):
    from openea_amd import ops
    dev = ops.device()
    z = np.load(GOLDEN)
    (ent, rel, m1, m2), batches, a1, a2 = fixture_case(z, case)
    lr = 0.01
    s = _setup(ent, rel, m1, m2, "SGD", dev, lr=lr)
    r0 = s["r"].clone()
    _step(s, batches, (a1, a2))
    loss, ref_loss = float(s["loss"].item()), float(z[case + "_loss"][0])
    print("%s: loss %.7f reference %.7f" % (case, loss, ref_loss))
    assert abs(loss - ref_loss) <= 2e-5 * abs(ref_loss)
    d = s["d"]
    for name, before, got in (("ent_embeds", ent, s["e"][:, :d]), ("mapping_matrix_1", m1, s["m1"]), ("mapping_matrix_2", m2, s["m2"])):
        g = (before.astype(np.float32).astype(np.float64) - got.cpu().numpy()) / lr          # SGD: the update IS lr * gradient
        ref = z["%s_grad_%s" % (case, name)]
        print("%s %s: max gradient deviation %.3g of max %.3g" % (case, name, np.abs(g - ref).max(), np.abs(ref).max()))
        assert np.abs(g - ref).max() <= 1e-3 * np.abs(ref).max(), name
    assert torch.equal(s["r"], r0)                                                       # rel_embeds: the same bits
    assert not s["e"][:, d:].any()


def _problem(rng, n_ent, dim, n_l, n_u, steps=3, disjoint=False):
    """tables + `steps` batches at a benchmark shape: KG1 = the first half of the ids, KG2 = the second, links (i, half + i);
    labelled links from the first 20 % of them, unlabelled from the rest; in every batch one entity repeated inside the labelled
    block and one labelled link also among the unlabelled; the last 100 entities of each KG in no batch.  disjoint: step s draws
    from the s-th slice of either range, so no entity is in the batches of two steps."""
    from openea_amd.modules.base.initializers import orthogonal_host, truncated_normal_host
    half = n_ent // 2
    ent = truncated_normal_host(rng, (n_ent, dim), 1.0 / np.sqrt(dim)).astype(np.float64)
    rel = truncated_normal_host(rng, (50, dim), 1.0 / np.sqrt(dim)).astype(np.float64)
    m1, m2 = (orthogonal_host(rng, (dim, dim)).astype(np.float64) for _ in range(2))
    n_links = half - 100
    n_train = n_links // 5
    batches = []
    for s in range(steps):
        if disjoint:
            cl, cu = n_train // steps, (n_links - n_train) // steps
            lab = s * cl + rng.choice(cl, n_l, replace=False)
            unl = n_train + s * cu + rng.choice(cu, n_u, replace=False)
        else:
            lab = rng.choice(n_train, n_l, replace=False)
            unl = n_train + rng.choice(n_links - n_train, n_u, replace=False)
        l1, l2, u1, u2 = lab.copy(), half + lab, unl.copy(), half + unl
        if n_l > 1:
            l1[1] = l1[0]
        if n_l and n_u:
            u1[0], u2[0] = l1[0], l2[0]
        batches.append((l1, l2, u1, u2))
    return ent, rel, m1, m2, batches


def _run_reference(ent, m1, m2, batches, lr=0.01):
    """three Adam steps of the float64 restatement -> tables, state, summed loss, per-step dense entity gradients"""
    tables = [ent.copy(), m1.copy(), m2.copy()]
    state = [(np.zeros_like(t), np.zeros_like(t)) for t in tables]
    loss, ent_grads = 0.0, []
    for t, b in enumerate(batches, 1):
        step_loss, grads = sea_reference_step(tables, state, b, lr, t, "Adam")
        loss += step_loss
        ent_grads.append(grads[0])
    return tables, state, loss, ent_grads


@pytest.mark.parametrize("n_ent,dim,n_l,n_u", [(30000, 8, 200, 800), (30000, 75, 200, 800), (30000, 100, 200, 800),
                                               (30000, 128, 200, 800), (200000, 100, 666, 2666)])
def test_adam_steps_equal_restatement(n_ent, dim, n_l, n_u):
    """three Adam steps at the EN-FR-15K-V1 / EN-FR-100K-V1 mapping shapes; dim = 75 has ld != dim.  Rows in no batch keep their
    bits and zero moments."""
    from _tol import assert_rows_close
    from openea_amd import ops
    dev = ops.device()
    rng = np.random.RandomState(dim + n_ent // 1000)
    ent, rel, m1, m2, batches = _problem(rng, n_ent, dim, n_l, n_u)
    s = _setup(ent, rel, m1, m2, "Adam", dev)
    r0 = s["r"].clone()
    for b in batches:
        _step(s, b)
    tables, state, loss_ref, ent_grads = _run_reference(ent, m1, m2, batches)
    loss = float(s["loss"].item())
    print("loss %.7f restatement %.7f" % (loss, loss_ref))
    assert abs(loss - loss_ref) <= 1e-4 * abs(loss_ref)
    used = np.unique(np.concatenate([np.concatenate(b) for b in batches]))
    small = np.all([np.abs(g) < TAU for g in ent_grads], axis=0)
    small[np.setdiff1d(np.arange(n_ent), used)] = False
    share = small.sum() / float(len(used) * dim)
    print("d=%d E=%d: %d of %d elements of batch rows under tau = %.0e in all steps (share %.3g, cap %.0e)"
          % (dim, n_ent, small.sum(), len(used) * dim, TAU, share, MASK_CAP))
    assert share <= MASK_CAP
    got = s["e"][:, :dim].cpu().numpy().astype(np.float64)
    got_cmp = np.where(small, tables[0], got)
    assert_rows_close(got_cmp, tables[0], "d=%d entity table" % dim)
    assert_rows_close(s["e_acc"][0, :, :dim].cpu().numpy(), state[0][0], "d=%d entity m" % dim)
    assert_rows_close(s["e_acc"][1, :, :dim].cpu().numpy(), state[0][1], "d=%d entity v" % dim)
    for name, g, ref in (("M1", s["m1"], tables[1]), ("M2", s["m2"], tables[2])):
        dev_max = np.abs(g.cpu().numpy() - ref).max()
        print("d=%d %s: max element deviation %.3g of max %.3g" % (dim, name, dev_max, np.abs(ref).max()))
        assert dev_max <= 1e-4 * np.abs(ref).max(), name
    unused = np.setdiff1d(np.arange(n_ent), used)
    assert len(unused) >= 200
    assert np.array_equal(got[unused], ent[unused].astype(np.float32))
    assert not s["e_acc"][:, torch.from_numpy(unused).to(dev)].any()
    assert torch.equal(s["r"], r0) and not s["r_acc"].any()


def test_mapping_optimiser_counts_its_own_steps(tmp_path):
    """two mapping epochs: t == 2 * triple_steps on the mapping trainer, whatever the triple trainer has counted"""
    from openea_amd.approaches import SEA
    from openea_amd.modules.base import initializers
    from openea_amd.modules.load.synth import make_kgs
    from openea_amd.run.default_args import get_args
    initializers.seed(5)
    m = SEA()
    m.set_args(get_args("SEA", output=str(tmp_path) + "/out/", training_data="synthetic/small/", dataset_division="fold1/", dim=32,
                        batch_size=2000, max_epoch=1))
    m.set_kgs(make_kgs("small", mode="mapping", seed=0))
    m.init()
    steps = 5
    m.launch_mapping_training_1epo(1, steps)
    m.launch_mapping_training_1epo(2, steps)
    assert m._mapping_trainer.t == 2 * steps and m._trainer.t == 0
    m.launch_triple_training_1epo(1, steps, None, None, None, None)
    assert m._mapping_trainer.t == 2 * steps and m._trainer.t == m._epochs.triple_steps
    assert m._mapping_trainer.ent_acc is not m._trainer.ent_acc


def _three_steps(dev, seed=11, disjoint=False):
    rng = np.random.RandomState(seed)
    ent, rel, m1, m2, batches = _problem(rng, 30000, 100, 200, 800, disjoint=disjoint)
    s = _setup(ent, rel, m1, m2, "Adam", dev)
    for b in batches:
        _step(s, b)
    torch.cuda.synchronize()
    return s


def test_matrices_have_the_same_bits_run_to_run():
    """The guarantee is per step: from the same entity rows, M1 / M2 and their moments come out with the same bits.  In the
    ordinary build an entity row that takes three or more gradient rows in a step (the repeated entity of every batch here) is
    summed by fp32 atomics in the order they arrive, so its last bits may differ run to run -- and with them a later step that
    gathers it again.  The steps here draw from disjoint slices of the links, so every step starts from rows that no earlier
    step's atomics touched (the dense Adam pass that moves every row is a fixed computation per element)."""
    from openea_amd import ops
    dev = ops.device()
    a, b = _three_steps(dev, disjoint=True), _three_steps(dev, disjoint=True)
    assert torch.equal(a["m1"], b["m1"]) and torch.equal(a["m2"], b["m2"]) and torch.equal(a["mst"], b["mst"])
    assert float(a["loss"].item()) == float(b["loss"].item())


DET_WORKER = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.environ["OEA_ROOT"]); sys.path.insert(0, os.path.join(os.environ["OEA_ROOT"], "tests"))
import torch
from openea_amd import ops
from test_sea_gpu import _three_steps
assert ops.deterministic()
dev = ops.device()
a, b = _three_steps(dev), _three_steps(dev)
same = all(torch.equal(a[k], b[k]) for k in ("m1", "m2", "mst", "e", "e_acc"))
print("RESULT SEA same_bits=%d" % int(same))
'''


def test_fixed_point_build_gives_the_same_bits():
    """libopenea_hip_det.so (OEA_STEP_DETERMINISTIC=1): two runs of three steps give bit-identical matrices, entity table and
    moments"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", DET_WORKER], env=dict(os.environ, OEA_ROOT=root, OEA_STEP_DETERMINISTIC="1"),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "RESULT SEA same_bits=1" in p.stdout, p.stdout


def test_epoch_call_equals_the_step_loop():
    """oea_sea_mapping_epoch == the same steps issued one by one: M1 / M2 bitwise, the entity table row by row (disjoint steps,
    for the reason given in test_matrices_have_the_same_bits_run_to_run)"""
    from _tol import assert_rows_close
    from openea_amd import ops
    dev = ops.device()
    rng = np.random.RandomState(23)
    ent, rel, m1, m2, batches = _problem(rng, 30000, 100, 200, 800, steps=3, disjoint=True)
    loop = _setup(ent, rel, m1, m2, "Adam", dev)
    for b in batches:
        _step(loop, b)
    s = _setup(ent, rel, m1, m2, "Adam", dev)
    packed = ops.to_ids(np.stack([np.concatenate(b) for b in batches]).astype(np.int32), dev)
    s["cfg"].opt_t = 1
    ops.sea_mapping_epoch(s["e"], s["e_acc"], s["r"], s["r_acc"], s["d"], packed, 200, 800, s["m1"], s["m2"], s["mst"], 2.5, 0.25,
                          s["cfg"], s["ws"], s["loss"], s["step_loss"])
    torch.cuda.synchronize()
    assert torch.equal(s["m1"], loop["m1"]) and torch.equal(s["m2"], loop["m2"]) and torch.equal(s["mst"], loop["mst"])
    assert float(s["loss"].item()) == float(loop["loss"].item())
    assert_rows_close(s["e"].cpu().numpy(), loop["e"].cpu().numpy(), "epoch call: entity table")
    assert_rows_close(s["e_acc"][0].cpu().numpy(), loop["e_acc"][0].cpu().numpy(), "epoch call: entity m")
    assert not torch.equal(s["m1"], torch.from_numpy(m1.astype(np.float32)).to(dev))


@pytest.mark.parametrize("bad", ["Adagrad", "Adadelta", "dim", "ld", "empty"])
def test_rejected_configurations_launch_nothing(bad):
    from openea_amd import ops
    from openea_amd._lib import OpenEAHipError
    dev = ops.device()
    rng = np.random.RandomState(1)
    dim = 129 if bad == "dim" else 30
    opt = bad if bad in ("Adagrad", "Adadelta") else "Adam"
    s = _setup(rng.randn(50, dim) * 0.1, rng.randn(6, dim) * 0.1, rng.randn(dim, dim) * 0.1, rng.randn(dim, dim) * 0.1, opt, dev)
    if bad == "Adagrad":
        s["e_acc"], s["r_acc"] = torch.full_like(s["e"], 0.1), torch.full_like(s["r"], 0.1)
        s["mst"] = torch.zeros((4, dim, dim), device=dev)
    if bad == "ld":                                             # ld = dim = 30, not a multiple of 4
        s["e"] = s["e"][:, :dim].contiguous()
        s["r"] = s["r"][:, :dim].contiguous()
        s["e_acc"], s["r_acc"] = (torch.zeros((2,) + tuple(t.shape), device=dev) for t in (s["e"], s["r"]))
        s["ws"] = ops.step_workspace(50, 6, dim, dev)
    batches = ([], [], [], []) if bad == "empty" else ([0, 1, 0], [20, 21, 22], [3, 4], [23, 24])
    e0, r0, m10, m20 = s["e"].clone(), s["r"].clone(), s["m1"].clone(), s["m2"].clone()
    ids = [ops.to_ids(np.asarray(b, np.int32), dev) for b in batches]
    s["cfg"].opt_t = 1
    with pytest.raises(OpenEAHipError):
        ops.sea_mapping_step(s["e"], s["d"], ids[0], ids[1], ids[2], ids[3], s["m1"], s["m2"], s["mst"], 2.5, 0.25, s["cfg"], s["ws"],
                             s["e"].shape[0], s["r"].shape[0], s["loss"], torch.empty(1 << 20, device=dev))
    packed = ops.to_ids(np.concatenate(batches).astype(np.int32)[None, :], dev)
    with pytest.raises(OpenEAHipError):
        ops.sea_mapping_epoch(s["e"], s["e_acc"], s["r"], s["r_acc"], s["d"], packed, len(batches[0]), len(batches[2]), s["m1"],
                              s["m2"], s["mst"], 2.5, 0.25, s["cfg"], s["ws"], s["loss"], s["step_loss"],
                              torch.empty(1 << 20, device=dev))
    torch.cuda.synchronize()
    assert torch.equal(s["e"], e0) and torch.equal(s["r"], r0) and torch.equal(s["m1"], m10) and torch.equal(s["m2"], m20)
    assert float(s["loss"].item()) == 0.0 and float(s["step_loss"].item()) == 0.0
    assert not s["ws"].any()


def test_end_to_end(tmp_path, capsys):
    from openea_amd.approaches import SEA
    from openea_amd.modules.base import initializers
    from openea_amd.modules.load.synth import make_kgs
    from openea_amd.run.default_args import get_args
    initializers.seed(20190719)
    kgs = make_kgs("small", mode="mapping", seed=0)
    d = 32
    model = SEA()
    model.set_args(get_args("SEA", output=str(tmp_path) + "/out/", training_data="synthetic/small/", dataset_division="fold1/",
                            dim=d, batch_size=2000, max_epoch=12, start_valid=4, eval_freq=4))
    model.set_kgs(kgs)
    model.init()
    assert model.mapping_mat is model.mapping_mat_1
    m1_0, m2_0 = model.mapping_mat_1.cpu().numpy().copy(), model.mapping_mat_2.cpu().numpy().copy()
    before = model.valid("hits1")
    model.run()
    after = model.valid("hits1")
    model.test()
    model.save()
    out = capsys.readouterr().out
    for line in ("avg. triple loss", "avg. mapping loss", "Training ends. Total time", "accurate results: hits@[1, 5, 10, 50]"):
        assert line in out, line
    print("hits@1 before %.2f after %.2f" % (before, after))
    assert after >= before - 1.0
    for t in (model.ent_embeds.var, model.rel_embeds.var, model.mapping_mat_1, model.mapping_mat_2):
        assert torch.isfinite(t).all()
    for name, init in (("mapping_mat", m1_0), ("rev_mapping_mat", m2_0)):
        saved = np.load(model.out_folder + name + ".npy")
        assert saved.shape == (d, d) and not np.array_equal(saved, init), name
    ent = np.load(model.out_folder + "ent_embeds.npy")
    assert ent.shape == (kgs.entities_num, d) and ent.dtype == np.float32
    np.testing.assert_allclose(np.linalg.norm(ent, axis=1), 1.0, rtol=1e-5)
    assert model._mapping_trainer.t == model._trainer.t > 0
