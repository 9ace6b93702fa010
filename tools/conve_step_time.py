"""Time of one ConvE training step (oea_log_uniform_sample + oea_conve_step) at the EN-FR-15K-V1 and EN-FR-100K-V1 sharing
shapes, next to the reference's formulation composed in torch (whole-table l2_normalize every step as TF does, the three affine
batch norms, conv2d, the dense layer and the sampled softmax written out, autograd, torch.optim.Adam over the fourteen variables)
-- the comparison leg, never the product path.

    python tools/conve_step_time.py [--dim 100] [--warmup 10] [--steps 50] [--torch-steps 10] [--shapes 15K,100K] [--out FILE]

Workload per shape: E entities, B positives per batch (500 at 15K, 5,000 at 100K: the shipped args files), S = 4,096 candidates,
F = 32 filters, keep_prob 0.7, heads under a Zipf law, labels uniform.  Device timing: HIP events around `steps` consecutive calls
after `warmup` calls, for the sampler alone, the gradient phase, the apply phase (dense Adam over the fourteen variables) and the
whole step as the trainer runs it.  The split inside the gradient phase is a kernel trace's business
(profiles/conve_step_kernel_stats_{15K,100K}.csv).  Both legs are fed the same sampled ids; the torch leg multiplies by the masks
of step 0 (the project's Philox definition, restated on the host) as given tensors, which leaves drawing them out of its time.
Prints one JSON line per shape."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from proje_step_time import N_SAMPLED, SHAPES, l2n, timed  # noqa: E402

FILTERS, KEEP, SEED = 32, 0.7, 7
BN_C = 1.0 / np.sqrt(1.0 + 1e-3)


def conve_torch_loss(tv, pos, sampled, log_q_s, log_q_t, m0, m1, x, y):
    ent, rel, w, b, g1, b1, kern, cb, g2, b2, fcw, fcb, g3, b3 = tv
    h, r, t = pos[:, 0], pos[:, 1], pos[:, 2]
    n = pos.shape[0]
    img = torch.cat([l2n(ent)[h].view(n, 1, x, y), l2n(rel)[r].view(n, 1, x, y)], 2)
    s = (img * (g1 * BN_C) + b1) / KEEP * m0
    z1 = torch.nn.functional.conv2d(s, kern.view(3, 3, 1, -1).permute(3, 2, 0, 1), cb, padding=1)
    a = torch.relu(z1 * (g2 * BN_C).view(1, -1, 1, 1) + b2.view(1, -1, 1, 1)) / KEEP * m1
    xo = torch.relu(a.reshape(n, -1) @ fcw + fcb) * (g3 * BN_C) + b3
    true = (xo * w[t]).sum(1) + b[t] - log_q_t
    samp = xo @ w[sampled].t() + b[sampled] - log_q_s
    sp = torch.nn.functional.softplus
    return sp(-true).sum() + sp(samp).sum()


def run(shape, a):
    from openea_amd import ops
    from openea_amd.modules.base.initializers import xavier_host
    from test_conve_cpu import dropout_masks
    dev = ops.device()
    name, E, R, B = SHAPES[shape]
    d, S, F = a.dim, N_SAMPLED, FILTERS
    x, y = ops.dim_factorization(d)
    K = 2 * d * F
    rng = np.random.RandomState(0)
    n_batches = a.warmup + max(a.steps, a.torch_steps + 3)
    p = 1.0 / np.arange(1, E + 1) ** 1.1
    pos = np.stack([rng.choice(E, (n_batches, B), p=p / p.sum()), rng.randint(0, R, (n_batches, B)),
                    rng.randint(0, E, (n_batches, B))], 2).astype(np.int32)
    pos_d = ops.to_ids(pos, dev)
    uni = lambda shp, fi, fo: rng.uniform(-np.sqrt(6.0 / (fi + fo)), np.sqrt(6.0 / (fi + fo)), shp).astype(np.float32)   # noqa: E731
    hosts = [xavier_host(rng, (E, d)), xavier_host(rng, (R, d)), xavier_host(rng, (E, d)), xavier_host(rng, (E,)),
             np.ones(y, np.float32), np.zeros(y, np.float32), uni((9 * F,), 9, 9 * F), np.zeros(F, np.float32), np.ones(F, np.float32),
             np.zeros(F, np.float32), uni((K, d), K, d), np.zeros(d, np.float32), np.ones(d, np.float32), np.zeros(d, np.float32)]

    # ---- device step ------------------------------------------------------------------------------------------------------
    v = [ops.to_table(h, dev=dev) if h.ndim == 2 else ops.to_vec(h, dev) for h in hosts]
    m, w = [torch.zeros_like(t) for t in v], [torch.zeros_like(t) for t in v]
    sampler = ops.LogUniformSampler(E, S, SEED, dev)
    ws = ops.conve_workspace(E, R, d, v[0].shape[1], F, B, S, dev)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    ids, tries, lq = sampler.sample(0)

    def phase(ph):
        return lambda s: ops.conve_step(v, m, w, d, F, KEEP, SEED, pos_d[s], ids, lq, tries, s, s + 1, 0.001, ws, loss, phase=ph,
                                        check_ids=False)

    def whole(s):
        i, t, q = sampler.sample(s)
        ops.conve_step(v, m, w, d, F, KEEP, SEED, pos_d[s], i, q, t, s, s + 1, 0.001, ws, loss, check_ids=False)

    ms_sampler = timed(lambda s: sampler.sample(s), a.warmup, a.steps)
    ms_grad = timed(phase(ops.PHASE_GRAD), a.warmup, a.steps)
    ms_apply = timed(phase(ops.PHASE_APPLY), a.warmup, a.steps)
    ms_step = timed(whole, a.warmup, a.steps)
    gflop = 3 * 2.0 * B * K * d / 1e9
    res = dict(metric="conve_step", shape=name, dim=d, batch=B, n_sampled=S, filters=F, keep_prob=KEEP, n_ent=E, n_rel=R,
               device_ms_per_step=round(ms_step, 4), sampler_ms=round(ms_sampler, 4), grad_phase_ms=round(ms_grad, 4),
               adam_ms=round(ms_apply, 4), adam_share=round(ms_apply / ms_step, 3), conv_dense_gflop_per_step=round(gflop, 3),
               nce_gflop_per_step=round(3 * 2.0 * B * S * d / 1e9, 3),
               conv_dense_tflops_of_grad_phase=round(gflop / ms_grad, 2), loss_finite=bool(np.isfinite(loss.item())))

    # ---- comparison leg: the reference's formulation composed in torch ---------------------------------------------------
    if a.torch_steps > 0:
        tv = [torch.from_numpy(np.asarray(h, np.float32)).to(dev).requires_grad_(True) for h in hosts]
        opt = torch.optim.Adam(tv, lr=0.001, eps=1e-8)
        ids_l = ids.long()
        cls = torch.arange(E, device=dev, dtype=torch.float64)
        log_q_all = torch.log(-torch.expm1(float(tries.item()) * torch.log1p(-(torch.log(cls + 2) - torch.log(cls + 1)) / np.log(E + 1.0)))).float()
        m0, m1 = dropout_masks(SEED, 0, B, d, F, KEEP)
        m0 = torch.from_numpy(m0.astype(np.float32)).to(dev).view(B, 1, 2 * x, y)
        m1 = torch.from_numpy(m1.astype(np.float32)).to(dev).view(B, F, 2 * x, y)

        def torch_step(s):
            pl = pos_d[s].long()
            opt.zero_grad(set_to_none=True)
            lv = conve_torch_loss(tv, pl, ids_l, log_q_all[ids_l], log_q_all[pl[:, 2]], m0, m1, x, y)
            lv.backward()
            opt.step()

        ms_torch = timed(torch_step, 3, a.torch_steps)
        res.update(torch_composed_ms_per_step=round(ms_torch, 4), speedup=round(ms_torch / ms_step, 2))
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=100)
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
