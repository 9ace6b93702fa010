"""Time of one TransR training step (oea_transr_step) at the EN-FR-15K-V1 shape, next to the reference's formulation composed
in torch (gathered [B, d, d] matrices, bmm, autograd, Adagrad) -- the comparison leg, never the product path.

    python tools/transr_step_time.py [--dim 100] [--batch 5000] [--warmup 20] [--steps 200] [--torch-steps 20]

Workload: a synthetic EN-FR-15K-V1-shaped KG pair (modules/load/synth.py, ids shared as in alignment_module 'sharing'), batches
of positives drawn from both KGs' triples, one uniform corruption of head or tail per positive, Adagrad, margin 1.5.  Device
timing: HIP events around `steps` consecutive steps after `warmup` steps.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=100)
    ap.add_argument("--batch", type=int, default=5000)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--torch-steps", type=int, default=20)
    a = ap.parse_args()
    from openea_amd import ops
    from openea_amd.modules.base.initializers import truncated_normal_host
    from openea_amd.modules.load.synth import make_kgs
    dev = ops.device()
    kgs = make_kgs("EN-FR-15K-V1", mode="sharing", seed=0)
    E, R, d, B = kgs.entities_num, kgs.relations_num, a.dim, a.batch
    triples = np.asarray(list(kgs.kg1.relation_triples_list) + list(kgs.kg2.relation_triples_list), np.int32)
    rng = np.random.RandomState(0)
    n_batches = a.warmup + a.steps
    pos = triples[rng.randint(0, len(triples), (n_batches, B))]
    neg = pos.copy()
    side = rng.randint(0, 2, (n_batches, B)) * 2
    bi, ri = np.meshgrid(np.arange(n_batches), np.arange(B), indexing="ij")
    neg[bi, ri, side] = rng.randint(0, E, (n_batches, B))
    pos_d, neg_d = ops.to_ids(pos, dev), ops.to_ids(neg, dev)
    ent_h = truncated_normal_host(rng, (E, d), 1.0 / np.sqrt(d))
    rel_h = truncated_normal_host(rng, (R, d), 1.0 / np.sqrt(d))
    mat_h = truncated_normal_host(rng, (R, d * d), 1.0 / d)

    # ---- device step ------------------------------------------------------------------------------------------------------
    ent, rel = ops.to_table(ent_h, dev=dev), ops.to_table(rel_h, dev=dev)
    mat = torch.from_numpy(np.ascontiguousarray(mat_h, np.float32)).to(dev)
    accs = [torch.full_like(t, 0.1) for t in (ent, rel, mat)]
    cfg = ops.make_step_cfg(loss="margin-based", loss_norm="L2", margin=1.5, optimizer="Adagrad", lr=0.01)
    ws = ops.step_workspace(E, R, ent.shape[1], dev)
    tws = ops.transr_workspace(E, R, d, B, dev)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)

    def dev_step(s):
        ops.transr_step(ent, accs[0], rel, accs[1], mat, accs[2], d, pos_d[s], neg_d[s], cfg, ws, tws, loss)

    for s in range(a.warmup):
        dev_step(s)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for s in range(a.steps):
        dev_step(a.warmup + s)
    t1.record()
    torch.cuda.synchronize()
    ms_dev = t0.elapsed_time(t1) / a.steps

    # ---- comparison leg: transr.py's formulation composed in torch ------------------------------------------------------
    tv = [torch.from_numpy(x.astype(np.float32)).to(dev).requires_grad_(True) for x in (ent_h, rel_h, mat_h)]
    tacc = [torch.full_like(v, 0.1) for v in tv]

    def l2n(x):
        return x * torch.rsqrt(torch.clamp((x * x).sum(1, keepdim=True), min=1e-12))

    def torch_step(s):
        p, n = pos_d[s].long(), neg_d[s].long()
        e, r = l2n(tv[0]), l2n(tv[1])
        pm = tv[2][p[:, 1]].view(-1, d, d)
        nm = tv[2][n[:, 1]].view(-1, d, d)
        ph = l2n(torch.bmm(pm, e[p[:, 0]].unsqueeze(2)).squeeze(2))
        pt = l2n(torch.bmm(pm, e[p[:, 2]].unsqueeze(2)).squeeze(2))
        nh = l2n(torch.bmm(nm, e[n[:, 0]].unsqueeze(2)).squeeze(2))
        nt = l2n(torch.bmm(nm, e[n[:, 2]].unsqueeze(2)).squeeze(2))
        lv = torch.relu(1.5 + ((ph + r[p[:, 1]] - pt) ** 2).sum(1) - ((nh + r[n[:, 1]] - nt) ** 2).sum(1)).sum()
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

    # ---- models from shapes ---------------------------------------------------------------------------------------------
    items = 4 * B
    r_present = len(np.unique(np.concatenate([pos[:, :, 1].ravel(), neg[:, :, 1].ravel()]))) if n_batches else R
    r_step = float(np.mean([len(np.unique(np.concatenate([pos[s, :, 1], neg[s, :, 1]]))) for s in range(min(n_batches, 20))]))
    flop = 3 * 2 * items * d * d                       # Y = X M^T, dX = dY M, dM = dY^T X
    mbytes = 4 * d * d * r_step * (2 + 4)             # M staged twice (fwd, bwd) + matrix and accumulator read and written
    ebytes = 4 * d * items * 2 + 4 * 4 * d * items    # entity rows gathered twice + y', dy written and read
    print(json.dumps(dict(metric="transr_step", dim=d, batch=B, n_ent=E, n_rel=R, relations_per_step=r_step,
                          relations_in_run=r_present, device_ms_per_step=round(ms_dev, 4),
                          device_triples_per_s=round(B / ms_dev * 1e3), torch_composed_ms_per_step=round(ms_torch, 4),
                          torch_triples_per_s=round(B / ms_torch * 1e3), speedup=round(ms_torch / ms_dev, 2),
                          gflop_per_step=round(flop / 1e9, 3), tflops=round(flop / ms_dev / 1e9, 2),
                          model_mb_matrices=round(mbytes / 1e6, 1), model_mb_rows=round(ebytes / 1e6, 1),
                          torch_gathered_mb=round(items / 2 * d * d * 4 / 1e6, 1),
                          loss_finite=bool(np.isfinite(loss.item())))))


if __name__ == "__main__":
    main()
