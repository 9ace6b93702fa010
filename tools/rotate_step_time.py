"""Time of one plain-RotatE training step (oea_rotate_step with neg_loss_div = k, fp64) at the EN-FR-15K-V1 and EN-FR-100K-V1
shapes, next to the reference's formulation composed in torch (models/semantic/rotate.py: whole-table l2_normalize of the three
float64 variables every step as TF does, autograd, dense Adam over every row) -- the comparison leg, never the product path.

    python tools/rotate_step_time.py [--dim 100] [--k 10] [--warmup 10] [--steps 50] [--torch-steps 10] [--shapes 15K,100K]

Workload per shape: a synthetic KG pair of that shape (modules/load/synth.py, ids shared as in alignment_module 'sharing'),
batches of positives drawn from both KGs' triples (5,000 at 15K, 20,000 at 100K: rotate_args_*.json), k uniform corruptions of
head or tail per positive, gamma 12, Adam.  Device timing: HIP events around `steps` consecutive steps after `warmup` steps; the
split into the triple kernel (PHASE_GRAD: rotate_triples + the fold of the relation copies) and the dense Adam over the
[2E, ld] and [R, ld] tables (PHASE_APPLY) is timed in a second pass of the same batches.  Prints one JSON line per shape."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"15K": ("EN-FR-15K-V1", 5000), "100K": ("EN-FR-100K-V1", 20000)}
GAMMA, LR = 12.0, 0.1


def l2n(x):
    return x * torch.rsqrt(torch.clamp((x * x).sum(1, keepdim=True), min=1e-12))


def rotate_torch_loss(tv, p, n, phase_scale, k):
    re, im, rel = l2n(tv[0]), l2n(tv[1]), l2n(tv[2])

    def dist(tr):
        h, r, t = tr[:, 0], tr[:, 1], tr[:, 2]
        theta = rel[r] * phase_scale
        rr, ir = torch.cos(theta), torch.sin(theta)
        a = re[h] * rr - im[h] * ir - re[t]
        b = re[h] * ir + im[h] * rr - im[t]
        return torch.stack([a, b]).norm(dim=0).sum(-1)
    logsig = torch.nn.functional.logsigmoid
    return -logsig(GAMMA - dist(p)).sum() - logsig(dist(n) - GAMMA).sum() / k


def _timed(fn, n, t0, t1):
    t0.record()
    for s in range(n):
        fn(s)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / n


def run(shape, a):
    from openea_amd import ops
    from openea_amd.modules.load.synth import make_kgs
    dev = ops.device()
    name, B = SHAPES[shape]
    kgs = make_kgs(name, mode="sharing", seed=0)
    E, R, d, k = kgs.entities_num, kgs.relations_num, a.dim, a.k
    triples = np.asarray(list(kgs.kg1.relation_triples_list) + list(kgs.kg2.relation_triples_list), np.int32)
    rng = np.random.RandomState(0)
    n_batches = a.warmup + a.steps
    pos = triples[rng.randint(0, len(triples), (n_batches, B))]
    neg = np.repeat(pos, k, axis=1)                                           # neg[s, p*k:(p+1)*k] corrupt pos[s, p]
    side = rng.randint(0, 2, (n_batches, B * k)) * 2
    bi, ri = np.meshgrid(np.arange(n_batches), np.arange(B * k), indexing="ij")
    neg[bi, ri, side] = rng.randint(0, E, (n_batches, B * k))
    pos_d, neg_d = ops.to_ids(pos, dev), ops.to_ids(neg, dev)
    hosts = [rng.uniform(0.0, 1.0, (E, d)).astype(np.float32) for _ in range(2)] + [rng.uniform(0.0, 1.0, (R, d)).astype(np.float32)]

    # ---- device step ------------------------------------------------------------------------------------------------------
    ent, rel = ops.to_table64(np.concatenate(hosts[:2]), dev), ops.to_table64(hosts[2], dev)
    se, sr = ops.rotate_state(ent, "Adam"), ops.rotate_state(rel, "Adam")
    cfg = ops.make_rotate_cfg(GAMMA, d, True, True, "Adam", LR, neg_loss_div=k)
    ws = ops.rotate_workspace(E, R, ent.shape[1], dev)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    count = [0]

    def dev_phase(s, phase):
        ops.rotate_step(ent, se, rel, sr, d, pos_d[s], neg_d[s], k, cfg, ws, loss, phase=phase)

    def dev_step(s):
        count[0] += 1
        cfg.t = count[0]
        dev_phase(s, ops.PHASE_BOTH)

    for s in range(a.warmup):
        dev_step(s)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms_dev = _timed(lambda s: dev_step(a.warmup + s), a.steps, t0, t1)
    # the split: the same batches once more, each phase between its own pair of events (the steps go on training)
    ms_grad = ms_apply = 0.0
    for s in range(a.steps):
        count[0] += 1
        cfg.t = count[0]
        for phase in (ops.PHASE_GRAD, ops.PHASE_APPLY):
            t0.record()
            dev_phase(a.warmup + s, phase)
            t1.record()
            torch.cuda.synchronize()
            if phase == ops.PHASE_GRAD:
                ms_grad += t0.elapsed_time(t1) / a.steps
            else:
                ms_apply += t0.elapsed_time(t1) / a.steps

    # ---- comparison leg: the reference's formulation composed in torch ---------------------------------------------------
    tv = [torch.from_numpy(x.astype(np.float64)).to(dev).requires_grad_(True) for x in hosts]
    m = [torch.zeros_like(v) for v in tv]
    vv = [torch.zeros_like(v) for v in tv]
    tcount = [0]

    def torch_step(s):
        tcount[0] += 1
        t = tcount[0]
        lv = rotate_torch_loss(tv, pos_d[s].long(), neg_d[s].long(), float(cfg.phase_scale), k)
        grads = torch.autograd.grad(lv, tv)
        lr_t = LR * np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t)
        with torch.no_grad():
            for v, mi, vi, g in zip(tv, m, vv, grads):
                mi.mul_(0.9).add_(g, alpha=0.1)
                vi.mul_(0.999).addcmul_(g, g, value=0.001)
                v.sub_(lr_t * mi / (vi.sqrt() + 1e-8))

    for s in range(3):
        torch_step(s)
    ms_torch = _timed(lambda s: torch_step(3 + s), a.torch_steps, t0, t1)

    res = dict(metric="rotate_step", model="RotatE", shape=name, dim=d, k=k, batch=B, n_ent=E, n_rel=R,
               device_ms_per_step=round(ms_dev, 4), device_triples_per_s=round(B * (k + 1) / ms_dev * 1e3),
               grad_phase_ms=round(ms_grad, 4), apply_phase_ms=round(ms_apply, 4),
               table_bytes_streamed_by_adam=int((2 * E + R) * ent.shape[1] * 8 * 8),      # var, m, v read + written, scratch read + zeroed
               torch_composed_ms_per_step=round(ms_torch, 4), speedup=round(ms_torch / ms_dev, 2),
               loss_finite=bool(np.isfinite(loss.item())))
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=100)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--torch-steps", type=int, default=10)
    ap.add_argument("--shapes", default="15K,100K")
    ap.add_argument("--out", default=None, help="also write the results as a JSON list here")
    a = ap.parse_args()
    out = [run(s, a) for s in a.shapes.split(",")]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
