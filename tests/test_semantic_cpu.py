"""HolE and SimplE without a GPU: a float64 restatement of both losses (CPU torch autograd) against the reference's own graphs
(tests/golden/semantic_graph.npz, make_semantic_golden.py), the direct circular correlation against the FFT form, and the
argument contract.  The GPU tests (test_semantic_gpu.py) hold the device step to this restatement at shapes the
finite-difference fixture cannot reach."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "semantic_graph.npz")
HOLE_VARS = ("ent_embeds", "rel_embeds")
SIMPLE_VARS = ("head_ent_embeds", "tail_ent_embeds", "rel_embeds1", "rel_embeds2")
CASES = ["hole_d5", "hole_d16", "hole_k3", "simple_d5", "simple_d16"]


def _l2n(x):
    """tf.nn.l2_normalize(x, 1): x * rsqrt(max(sum x^2, 1e-12))"""
    return x * torch.rsqrt(torch.clamp((x * x).sum(1, keepdim=True), min=1e-12))


def ccorr_fft(h, t):
    """hole.py:50-53: real(ifft(conj(fft(h)) * fft(t)))"""
    return torch.fft.ifft(torch.conj(torch.fft.fft(h)) * torch.fft.fft(t)).real


def ccorr_direct(h, t):
    """c[k] = sum_i h[i] t[(i + k) mod d]"""
    d = h.shape[1]
    idx = (torch.arange(d)[:, None] + torch.arange(d)[None, :]) % d          # [i, k]
    return torch.einsum("ni,nik->nk", h, t[:, idx])


def _ids(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.long)


def hole_loss(ent, rel, pos, neg, margin, k):
    """hole.py:55-84 in float64: both tables normalised at lookup, the relation row once more, margin against the mean of the
    k negatives neg[p*k:(p+1)*k]"""
    e, r = _l2n(ent), _l2n(rel)
    pos, neg = _ids(pos), _ids(neg)

    def score(tr):
        c = ccorr_fft(e[tr[:, 0]], e[tr[:, 2]])
        return -torch.sigmoid((_l2n(r[tr[:, 1]]) * c).sum(1))
    return torch.relu(margin + score(pos) - score(neg).view(-1, k).mean(1)).sum()


def simple_loss(head, tail, rel1, rel2, pos, neg):
    """simple.py:62-88 in float64"""
    H, T, R1, R2 = _l2n(head), _l2n(tail), _l2n(rel1), _l2n(rel2)
    pos, neg = _ids(pos), _ids(neg)

    def score(tr):
        h, r, t = tr[:, 0], tr[:, 1], tr[:, 2]
        return ((_l2n(H[h] * R1[r]) * T[t]).sum(1) + (_l2n(H[t] * R2[r]) * T[h]).sum(1)) / 2
    return torch.nn.functional.softplus(-score(pos)).sum() + torch.nn.functional.softplus(score(neg)).sum()


def semantic_grads(model, tables, pos, neg, margin=0.0, k=1):
    """-> loss, [d loss / d table] (float64 numpy); model 'HolE' (ent, rel) or 'SimplE' (head, tail, rel1, rel2)"""
    vs = [torch.tensor(np.asarray(v, np.float64), requires_grad=True) for v in tables]
    loss = hole_loss(*vs, pos, neg, margin, k) if model == "HolE" else simple_loss(*vs, pos, neg)
    grads = torch.autograd.grad(loss, vs)
    return float(loss.detach()), [g.numpy() for g in grads]


def semantic_reference_step(model, tables, accs, pos, neg, lr, margin=0.0, k=1, optimizer="Adagrad"):
    """one optimiser step of every table in place (float64).  TF's update of the normalised tables equals the dense update
    below: a zero gradient leaves a row and its accumulator unchanged.  -> the batch loss"""
    loss, grads = semantic_grads(model, tables, pos, neg, margin, k)
    for v, a, g in zip(tables, accs, grads):
        if optimizer == "Adagrad":
            a += g * g
            v -= lr * g / np.sqrt(a)
        else:
            v -= lr * g
    return loss


def fixture_case(z, case):
    """-> model, tables, pos, neg, margin, k of one fixture case"""
    model = "HolE" if case.startswith("hole") else "SimplE"
    names = HOLE_VARS if model == "HolE" else SIMPLE_VARS
    tables = [z["%s_var_%s" % (case, n)] for n in names]
    return model, tables, z[case + "_pos"], z[case + "_neg"], float(z[case + "_margin"][0]), int(z[case + "_shape"][3])


@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_reference_graph(case):
    z = np.load(GOLDEN)
    model, tables, pos, neg, margin, k = fixture_case(z, case)
    loss, grads = semantic_grads(model, tables, pos, neg, margin, k)
    ref_loss = z[case + "_loss"][0]
    assert abs(loss - ref_loss) <= 1e-6 * abs(ref_loss)
    names = HOLE_VARS if model == "HolE" else SIMPLE_VARS
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
        assert (np.repeat(pos[:, 1], k) != neg[:, 1]).any(), case                  # a negative with another relation
        assert (pos[:, 0] == pos[:, 2]).any(), case                                # h == t
        assert len(np.unique(np.concatenate([pos[:, 0], pos[:, 2]]))) < 2 * len(pos), case
    assert [tuple(z[c + "_shape"]) for c in CASES] == [(14, 4, 5, 1), (24, 5, 16, 1), (24, 5, 16, 3), (14, 4, 5, 1), (24, 5, 16, 1)]


def test_direct_circular_correlation_equals_the_fft_form():
    rng = np.random.RandomState(3)
    h, t = torch.tensor(rng.randn(7, 100)), torch.tensor(rng.randn(7, 100))
    np.testing.assert_allclose(ccorr_direct(h, t).numpy(), ccorr_fft(h, t).numpy(), rtol=0, atol=1e-12)


SHIPPED = {
    # run/args/hole_args_{15K,100K}.json
    "HolE": dict(embedding_module="HolE", alignment_module="sharing", dim=100, init="xavier", ent_l2_norm=True, rel_l2_norm=True,
                 loss_norm="L2", margin=0.2, neg_sampling="uniform", neg_triple_num=1, learning_rate=0.01, optimizer="Adagrad",
                 max_epoch=2000, batch_size=5000, start_valid=100, eval_freq=10, stop_metric="hits1", eval_metric="inner",
                 csls=10, top_k=[1, 5, 10, 50], is_save=True, eval_norm=False),
    # run/args/simple_args_{15K,100K}.json
    "SimplE": dict(embedding_module="SimplE", alignment_module="sharing", dim=100, init="xavier", ent_l2_norm=True,
                   rel_l2_norm=True, neg_sampling="uniform", neg_triple_num=1, learning_rate=0.01, optimizer="Adagrad",
                   max_epoch=2000, batch_size=5000, start_valid=10, eval_freq=10, stop_metric="hits1", eval_metric="inner",
                   csls=10, top_k=[1, 5, 10, 50], is_save=True, eval_norm=True),
}
SHIPPED_100K = {"HolE": dict(batch_size=20000), "SimplE": dict(batch_size=20000, start_valid=50)}


@pytest.mark.parametrize("name", ["HolE", "SimplE"])
@pytest.mark.parametrize("scale", ["15K", "100K"])
def test_args_match_the_shipped_run_configs(name, scale):
    from openea_amd.run.default_args import get_args
    a = get_args(name, scale)
    expect = dict(SHIPPED[name], **(SHIPPED_100K[name] if scale == "100K" else {}))
    for k, v in expect.items():
        assert getattr(a, k) == v, k


@pytest.mark.parametrize("name,bad", [("HolE", dict(init="normal")), ("HolE", dict(alignment_module="swapping")),
                                      ("HolE", dict(neg_sampling="truncated")), ("HolE", dict(optimizer="SGD")),
                                      ("HolE", dict(eval_metric="euclidean")), ("HolE", dict(loss_norm="L1")),
                                      ("HolE", dict(ent_l2_norm=False)), ("HolE", dict(rel_l2_norm=False)),
                                      ("HolE", dict(margin=0.0)),
                                      ("SimplE", dict(init="normal")), ("SimplE", dict(alignment_module="mapping")),
                                      ("SimplE", dict(neg_sampling="truncated")), ("SimplE", dict(optimizer="Adam")),
                                      ("SimplE", dict(eval_metric="manhattan")), ("SimplE", dict(ent_l2_norm=False)),
                                      ("SimplE", dict(rel_l2_norm=False))])
def test_check_args_rejects_each_asserted_key(name, bad):
    """hole.py:28-36, simple.py:28-34"""
    from openea_amd.models import semantic
    from openea_amd.run.default_args import get_args
    m = getattr(semantic, name)()
    m.args = get_args(name)
    m._check_args()
    m.args = get_args(name, **bad)
    with pytest.raises(AssertionError):
        m._check_args()


def test_semantic_trainer_rejects_other_optimizers():
    from openea_amd.models.semantic.semantic_trainer import SemanticTrainer
    with pytest.raises(NotImplementedError, match="Adagrad"):
        SemanticTrainer(0, None, None, None, "Adam")
