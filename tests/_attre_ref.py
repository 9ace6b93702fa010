"""Restatements of AttrE's three device pieces, for test_attre_cpu.py and test_attre_gpu.py.  Everything here runs on the CPU.

  composition   weights(L) is the closed form w_p = sum_{m = p + 1 .. L} 1 / m; weights_loop(L) walks the reference's while_loop
                over the reversed stack (attre.py:94-109) on unit vectors.
  char_loss     the character loss (attre.py:166-187 + losses.py) in torch, in the dtype of the tables it is given: float64 is the
                reference, the same lines on float32 tensors are the float32 run that tests/_grads.gradient_check measures E32 from.
  joint_loss    attre.py:189-190.
  sample_heads  numpy restatement of oea_attre_sample_heads, bit for bit.
  replay        SGD / Adagrad steps on the gradients above."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from test_proje_cpu import philox4x32_10  # noqa: E402


def weights(L):
    return np.array([sum(1.0 / m for m in range(p + 1, L + 1)) for p in range(L)], np.float64)


def weights_loop(L):
    """calculate_ngram_weight on a batch of one whose character vectors are the unit vectors: the result is the weight row"""
    stacked = np.eye(L)[None, :, :]                       # [1, L, L]: character p is e_p
    stacked = stacked[:, ::-1, :]                         # tf.reverse(stacked_tensor, [1])
    index, summation = L, np.zeros((1, L))
    while index > 0:
        processed = stacked[:, index - 1:, :]             # tf.slice(stacked_tensor, [0, index - 1, 0], [-1, -1, -1])
        summation = summation + processed.mean(1)
        index -= 1
    return summation[0]


def _l2n(t, on):
    return t / torch.sqrt(torch.clamp((t * t).sum(1, keepdim=True), min=1e-12)) if on else t


def _ids(a):
    return torch.as_tensor(np.asarray(a, np.int64))


def _score(x, l1):
    return x.abs().sum(1) if l1 else (x * x).sum(1)


def char_loss(ent, attr, chars, b):
    """b: pos [n, 3] (e, a, value row), neg_heads [n k], value_chars [V, L], loss, l1, margin, pos_margin, neg_margin, balance,
    ent_l2n, attr_l2n, char_l2n -> the batch loss (a torch scalar of the tables' dtype)"""
    pos, k = np.asarray(b["pos"]), b["k"]
    L = b["value_chars"].shape[1]
    w = torch.tensor(weights(L), dtype=ent.dtype)
    E, A, C = _l2n(ent, b["ent_l2n"]), _l2n(attr, b["attr_l2n"]), _l2n(chars, b["char_l2n"])
    ids = _ids(b["value_chars"][pos[:, 2]])                                   # [n, L]
    v = (C[ids] * w[None, :, None]).sum(1)
    wa = A[_ids(pos[:, 1])]
    ps = _score(E[_ids(pos[:, 0])] + wa - v, b["l1"])
    ns = _score(E[_ids(b["neg_heads"])] + wa.repeat_interleave(k, 0) - v.repeat_interleave(k, 0), b["l1"])
    if b["loss"] == "margin-based":
        assert k == 1
        return torch.relu(b["margin"] + ps - ns).sum()
    if b["loss"] == "logistic":
        # losses.py:70-71 literally in float64; float32 overflows in exp above a score of 88 (|v| reaches L), so the float32 run
        # takes the stable form of the same function
        sp = (lambda x: torch.log(1 + torch.exp(x))) if ent.dtype == torch.float64 else torch.nn.functional.softplus
        return sp(ps).sum() + sp(-ns).sum()
    assert b["loss"] == "limited"
    return torch.relu(ps - b["pos_margin"]).sum() + b["balance"] * torch.relu(b["neg_margin"] - ns).sum()


def char_grads(tables, b, dtype=np.float64):
    """-> loss, [d / d ent_ce, d / d attr, d / d chars] as float64 arrays (of float32 values when dtype is float32)"""
    vs = [torch.tensor(np.asarray(t, dtype), requires_grad=True) for t in tables]
    loss = char_loss(vs[0], vs[1], vs[2], b)
    grads = torch.autograd.grad(loss, vs, allow_unused=True)
    return float(loss.detach()), [np.zeros(v.shape) if g is None else g.numpy().astype(np.float64) for v, g in zip(vs, grads)]


def joint_loss(ent, ce, on, entities=None):
    """entities: the step's entity list (a row named twice counts twice); None: every row once"""
    ids = _ids(np.arange(len(ent)) if entities is None else entities)
    return (1 - (_l2n(ent, on)[ids] * _l2n(ce, on)[ids]).sum(1, keepdim=True)).sum()


def joint_grads(ent, ce, on, dtype=np.float64, entities=None):
    vs = [torch.tensor(np.asarray(t, dtype), requires_grad=True) for t in (ent, ce)]
    loss = joint_loss(vs[0], vs[1], on, entities)
    return float(loss.detach()), [g.numpy().astype(np.float64) for g in torch.autograd.grad(loss, vs)]


def optimiser_step(tables, grads, accs, optimizer, lr):
    """SGD, or tf.train.AdagradOptimizer (acc += g^2; v -= lr g / sqrt(acc)) -> new tables, new accumulators (float64)"""
    if optimizer == "SGD":
        return [t - lr * g for t, g in zip(tables, grads)], accs
    accs = [a + g * g for a, g in zip(accs, grads)]
    return [t - lr * g / np.sqrt(a) for t, g, a in zip(tables, grads, accs)], accs


def sample_heads(pos, n_split, k, lists, ent_poss, seed, step, pos_offset=0):
    """oea_attre_sample_heads: out[p k + s] = list[j], j = mulhi(word 0 of Philox(p + pos_offset, step, 0, s), n - 1), stepped over
    the head's own position"""
    pos = np.asarray(pos)
    n = len(pos)
    out = np.empty((n, k), np.int32)
    p = (np.arange(n, dtype=np.uint64) + np.uint64(pos_offset)) & np.uint64(0xFFFFFFFF)
    for s in range(k):
        word = philox4x32_10(p, step & 0xFFFFFFFF, 0, s, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)[:, 0].astype(np.uint64)
        for side, (lo, hi) in enumerate(((0, n_split), (n_split, n))):
            if hi <= lo:
                continue
            lst, ent_pos = np.asarray(lists[side]), np.asarray(ent_poss[side])
            own = ent_pos[pos[lo:hi, 0]].astype(np.int64)
            listed = own >= 0
            m = np.where(listed, len(lst) - 1, len(lst)).astype(np.uint64)
            j = ((word[lo:hi] * m) >> np.uint64(32)).astype(np.int64)
            j += (listed & (j >= own)).astype(np.int64)
            out[lo:hi, s] = lst[j]
    return out.reshape(-1)
