"""TransR without a GPU: a float64 restatement of the step (CPU torch autograd) against the reference's own graph
(tests/golden/transr_graph.npz, make_transr_golden.py), and the argument contract.  The GPU tests
(test_transr_gpu.py) hold the device step to this restatement at shapes the finite-difference fixture cannot reach."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transr_graph.npz")


def _l2n(x):
    """tf.nn.l2_normalize(x, 1): x * rsqrt(max(sum x^2, 1e-12))"""
    return x * torch.rsqrt(torch.clamp((x * x).sum(1, keepdim=True), min=1e-12))


def transr_loss(ent, rel, rel_matrix, pos, neg, margin, ent_l2_norm=True, rel_l2_norm=True):
    """transr.py:33-50 in float64: projected, normalised h / t per side with the side's own relation, margin loss over pairs.
    The projections are grouped by relation (the reference's gathered [B, d, d] matrices do not fit at the large shapes)."""
    d = ent.shape[1]
    e = _l2n(ent) if ent_l2_norm else ent
    r = _l2n(rel) if rel_l2_norm else rel
    pos, neg = torch.as_tensor(pos, dtype=torch.long), torch.as_tensor(neg, dtype=torch.long)
    ents = torch.cat([pos[:, 0], pos[:, 2], neg[:, 0], neg[:, 2]])
    rels = torch.cat([pos[:, 1], pos[:, 1], neg[:, 1], neg[:, 1]])
    mats = rel_matrix.view(-1, d, d)
    order = torch.argsort(rels, stable=True)
    rs, counts = torch.unique_consecutive(rels[order], return_counts=True)
    xs = torch.split(e[ents[order]], counts.tolist())
    y = torch.cat([xg @ mats[rr].T for xg, rr in zip(xs, rs.tolist())])[torch.argsort(order)]
    y = _l2n(y)
    n = pos.shape[0]
    ph, pt, nh, nt = y[:n], y[n:2 * n], y[2 * n:3 * n], y[3 * n:]
    pd = ((ph + r[pos[:, 1]] - pt) ** 2).sum(1)
    nd = ((nh + r[neg[:, 1]] - nt) ** 2).sum(1)
    return torch.relu(margin + pd - nd).sum()


def transr_grads(ent, rel, rel_matrix, pos, neg, margin, **kw):
    """-> loss, [d loss / d ent, d rel, d rel_matrix] (float64 numpy) at the given host tables"""
    vs = [torch.tensor(np.asarray(v, np.float64), requires_grad=True) for v in (ent, rel, rel_matrix)]
    loss = transr_loss(*vs, pos, neg, margin, **kw)
    grads = torch.autograd.grad(loss, vs)
    return float(loss.detach()), [g.numpy() for g in grads]


def transr_reference_step(tables, accs, pos, neg, margin, lr, optimizer="Adagrad"):
    """one optimiser step of the three variables in place (float64).  TF's sparse Adagrad on rel_matrix (duplicates summed,
    absent rows untouched) and its dense update of the normalised tables both equal the dense update below: a zero gradient
    leaves a row and its accumulator unchanged.  -> the batch loss"""
    loss, grads = transr_grads(*tables, pos, neg, margin)
    for v, a, g in zip(tables, accs, grads):
        if optimizer == "Adagrad":
            a += g * g
            v -= lr * g / np.sqrt(a)
        else:
            v -= lr * g
    return loss


@pytest.mark.parametrize("case", ["tiny", "d16"])
def test_restatement_equals_reference_graph(case):
    z = np.load(GOLDEN)
    tables = [z["%s_var_%s" % (case, n)] for n in ("ent_embeds", "rel_embeds", "rel_matrix")]
    loss, grads = transr_grads(*tables, z[case + "_pos"], z[case + "_neg"], float(z[case + "_margin"][0]))
    assert abs(loss - z[case + "_loss"][0]) <= 1e-9 * abs(z[case + "_loss"][0])
    for name, g in zip(("ent_embeds", "rel_embeds", "rel_matrix"), grads):
        ref = z["%s_grad_%s" % (case, name)]
        assert g.shape == ref.shape
        assert np.abs(g - ref).max() <= 1e-5 * np.abs(ref).max(), name
        assert np.abs(ref).max() > 0, name


def test_fixture_covers_the_cases():
    z = np.load(GOLDEN)
    pos, neg = z["d16_pos"], z["d16_neg"]
    assert (pos[:, 1] != neg[:, 1]).any()                           # a negative with another relation
    assert len(np.unique(pos[:, 1])) < len(pos)                     # repeated relations
    assert len(np.unique(np.concatenate([pos[:, 0], pos[:, 2]]))) < 2 * len(pos)
    assert tuple(z["d16_shape"]) == (24, 5, 16) and tuple(z["tiny_shape"]) == (14, 4, 5)
    # rows absent from the batch have a zero gradient (the sparse update leaves them alone)
    g = z["d16_grad_rel_matrix"]
    absent = sorted(set(range(5)) - set(pos[:, 1]) - set(neg[:, 1]))
    assert all(np.abs(g[r]).max() == 0 for r in absent)


def test_transr_args_match_the_shipped_run_config():
    """run/args/transr_args_15K.json"""
    from openea_amd.run.default_args import get_args
    a = get_args("TransR")
    expect = dict(embedding_module="TransR", alignment_module="sharing", dim=100, init="normal", ent_l2_norm=True,
                  rel_l2_norm=True, loss_norm="L2", margin=1.5, loss="margin-based", neg_sampling="uniform", neg_triple_num=1,
                  learning_rate=0.01, optimizer="Adagrad", batch_size=5000, eval_metric="inner", eval_norm=False)
    for k, v in expect.items():
        assert getattr(a, k) == v, k


@pytest.mark.parametrize("bad", [dict(loss_norm="L1"), dict(loss="limited"), dict(optimizer="Adam"), dict(neg_triple_num=2),
                                 dict(alignment_module="swapping")])
def test_transr_argument_contract(bad):
    """transe.py:20-29, inherited by TransR"""
    from openea_amd.models.trans import TransR
    from openea_amd.run.default_args import get_args
    m = TransR()
    m.args = get_args("TransR")
    m._check_args()
    m.args = get_args("TransR", **bad)
    with pytest.raises(AssertionError):
        m._check_args()


def test_transr_trainer_rejects_other_optimizers():
    from openea_amd.models.trans.transr import TransRTrainer
    with pytest.raises(NotImplementedError, match="Adagrad"):
        TransRTrainer(None, None, None, None, "Adam")
