"""Time of one HolE / SimplE / DistMult training step (oea_semantic_step) at the EN-FR-15K-V1 and EN-FR-100K-V1 shapes, next to the
reference's formulation composed in torch (HolE: complex64 torch.fft; both: whole-table l2_normalize every step as TF does,
autograd, Adagrad) -- the comparison leg, never the product path.

    python tools/semantic_step_time.py [--dim 100] [--warmup 20] [--steps 100] [--torch-steps 10] [--shapes 15K,100K]

Workload per shape: a synthetic KG pair of that shape (modules/load/synth.py, ids shared as in alignment_module 'sharing'),
batches of positives drawn from both KGs' triples (5,000 at 15K, 20,000 at 100K: the shipped args files), one uniform
corruption of head or tail per positive, Adagrad, HolE margin 0.2 (DistMult: the mean over the 2 B labelled triples).  Device timing: HIP events around `steps` consecutive
steps after `warmup` steps.  Prints one JSON line per (model, shape)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"15K": ("EN-FR-15K-V1", 5000), "100K": ("EN-FR-100K-V1", 20000)}


def l2n(x):
    return x * torch.rsqrt(torch.clamp((x * x).sum(1, keepdim=True), min=1e-12))


def hole_torch_loss(tv, p, n):
    e, r = l2n(tv[0]), l2n(tv[1])

    def score(tr):
        h = e[tr[:, 0]].to(torch.complex64)
        t = e[tr[:, 2]].to(torch.complex64)
        c = torch.fft.ifft(torch.conj(torch.fft.fft(h)) * torch.fft.fft(t)).real
        return -torch.sigmoid((l2n(r[tr[:, 1]]) * c).sum(1))
    return torch.relu(0.2 + score(p) - score(n)).sum()


def simple_torch_loss(tv, p, n):
    H, T, R1, R2 = (l2n(v) for v in tv)

    def score(tr):
        h, r, t = tr[:, 0], tr[:, 1], tr[:, 2]
        return ((l2n(H[h] * R1[r]) * T[t]).sum(1) + (l2n(H[t] * R2[r]) * T[h]).sum(1)) / 2
    return torch.nn.functional.softplus(-score(p)).sum() + torch.nn.functional.softplus(score(n)).sum()


def distmult_torch_loss(tv, p, n):
    e, w = l2n(tv[0]), l2n(tv[1])
    tr = torch.cat([p, n])
    label = torch.cat([torch.ones(len(p), device=p.device), -torch.ones(len(n), device=p.device)])
    return torch.nn.functional.softplus(-label * (e[tr[:, 0]] * w[tr[:, 1]] * e[tr[:, 2]]).sum(1)).mean()


KINDS = {"HolE": "SEMANTIC_HOLE", "SimplE": "SEMANTIC_SIMPLE", "DistMult": "SEMANTIC_DISTMULT"}
TORCH_LOSS = {"HolE": hole_torch_loss, "SimplE": simple_torch_loss, "DistMult": distmult_torch_loss}


def run(model, shape, a):
    from openea_amd import ops
    from openea_amd.modules.base.initializers import xavier_host
    from openea_amd.modules.load.synth import make_kgs
    dev = ops.device()
    name, B = SHAPES[shape]
    kgs = make_kgs(name, mode="sharing", seed=0)
    E, R, d = kgs.entities_num, kgs.relations_num, a.dim
    triples = np.asarray(list(kgs.kg1.relation_triples_list) + list(kgs.kg2.relation_triples_list), np.int32)
    rng = np.random.RandomState(0)
    n_batches = a.warmup + a.steps
    pos = triples[rng.randint(0, len(triples), (n_batches, B))]
    neg = pos.copy()
    side = rng.randint(0, 2, (n_batches, B)) * 2
    bi, ri = np.meshgrid(np.arange(n_batches), np.arange(B), indexing="ij")
    neg[bi, ri, side] = rng.randint(0, E, (n_batches, B))
    pos_d, neg_d = ops.to_ids(pos, dev), ops.to_ids(neg, dev)
    n_tab = 2 if model == "SimplE" else 1
    hosts = [xavier_host(rng, (E, d)) for _ in range(n_tab)] + [xavier_host(rng, (R, d)) for _ in range(n_tab)]

    # ---- device step ------------------------------------------------------------------------------------------------------
    ent = ops.to_table(np.concatenate(hosts[:n_tab]), dev=dev)
    rel = ops.to_table(np.concatenate(hosts[n_tab:]), dev=dev)
    accs = [torch.full_like(t, 0.1) for t in (ent, rel)]
    cfg = ops.make_step_cfg(loss="margin-based", margin=0.2, optimizer="Adagrad", lr=0.01, neg_group_k=1)
    ws = ops.step_workspace(ent.shape[0], rel.shape[0], ent.shape[1], dev)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    kind = getattr(ops, KINDS[model])

    def dev_step(s):
        ops.semantic_step(kind, ent, accs[0], rel, accs[1], d, pos_d[s], neg_d[s], cfg, ws, loss)

    for s in range(a.warmup):
        dev_step(s)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for s in range(a.steps):
        dev_step(a.warmup + s)
    t1.record()
    torch.cuda.synchronize()
    ms_dev = t0.elapsed_time(t1) / a.steps

    # ---- comparison leg: the reference's formulation composed in torch ---------------------------------------------------
    tv = [torch.from_numpy(x.astype(np.float32)).to(dev).requires_grad_(True) for x in hosts]
    tacc = [torch.full_like(v, 0.1) for v in tv]
    torch_loss = TORCH_LOSS[model]

    def torch_step(s):
        lv = torch_loss(tv, pos_d[s].long(), neg_d[s].long())
        grads = torch.autograd.grad(lv, tv)
        with torch.no_grad():
            for v, acc, g in zip(tv, tacc, grads):
                acc.add_(g * g)
                v.sub_(0.01 * g / acc.sqrt())

    for s in range(3):
        torch_step(s)
    t0.record()
    for s in range(a.torch_steps):
        torch_step(3 + s)
    t1.record()
    torch.cuda.synchronize()
    ms_torch = t0.elapsed_time(t1) / a.torch_steps

    # ---- model from shapes: HolE 6 d^2 FLOP per scored triple (F, C, G) + 2 d^2 for the scoring pass --------------------------
    triples_per_step = 2 * B
    flop = (8 if model == "HolE" else 0) * d * d * triples_per_step
    res = dict(metric="semantic_step", model=model, shape=name, dim=d, batch=B, n_ent=E, n_rel=R,
               device_ms_per_step=round(ms_dev, 4), device_triples_per_s=round(B / ms_dev * 1e3),
               torch_composed_ms_per_step=round(ms_torch, 4), speedup=round(ms_torch / ms_dev, 2),
               loss_finite=bool(np.isfinite(loss.item())))
    if flop:
        res.update(gflop_per_step_upper=round(flop / 1e9, 3), tflops_upper=round(flop / ms_dev / 1e9, 2))
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--torch-steps", type=int, default=10)
    ap.add_argument("--shapes", default="15K,100K")
    ap.add_argument("--models", default="HolE,SimplE,DistMult")
    ap.add_argument("--out", default=None, help="also write the results as a JSON list here")
    a = ap.parse_args()
    out = [run(m, s, a) for s in a.shapes.split(",") for m in a.models.split(",")]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
