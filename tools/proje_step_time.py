"""Time of one ProjE training step (oea_log_uniform_sample + oea_proje_step) at the EN-FR-15K-V1 and EN-FR-100K-V1 sharing
shapes, next to the reference's formulation composed in torch (whole-table l2_normalize every step as TF does, batch norms and
the sampled softmax written out, autograd, torch.optim.Adam over the eight variables) -- the comparison leg, never the product
path.

    python tools/proje_step_time.py [--dim 100] [--warmup 10] [--steps 50] [--torch-steps 10] [--shapes 15K,100K] [--out FILE]

Workload per shape: E entities, B positives per batch (500 at 15K, 5,000 at 100K: the shipped args files), S = 4,096 candidates,
heads under a Zipf law, labels uniform.  Device timing: HIP events around `steps` consecutive calls after `warmup` calls, for the
sampler alone (its status read-back included), the gradient phase (projection + the two NCE sweeps), the apply phase (dense Adam
over the eight variables) and the whole step as the trainer runs it.  The projection / sweep split inside the gradient phase is a
kernel trace's business (profiles/proje_step_kernel_stats.csv).  Both legs are fed the same sampled ids.  Prints one JSON line per
shape."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"15K": ("EN-FR-15K-V1", 27000, 477, 500), "100K": ("EN-FR-100K-V1", 180000, 1300, 5000)}
N_SAMPLED = 4096


def l2n(x):
    return x * torch.rsqrt(torch.clamp((x * x).sum(1, keepdim=True), min=1e-12))


def bn(x, beta):
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    return (x - mean) * torch.rsqrt(var + 1e-3) + beta


def proje_torch_loss(tv, pos, sampled, log_q_s, log_q_t):
    ent, rel, w, b, beta_in, mlp_w, mlp_b, beta_out = tv
    h, r, t = pos[:, 0], pos[:, 1], pos[:, 2]
    x = bn((bn(l2n(ent)[h], beta_in) + bn(l2n(rel)[r], beta_in)) * mlp_w + mlp_b, beta_out)
    true = (x * w[t]).sum(1) + b[t] - log_q_t
    samp = x @ w[sampled].t() + b[sampled] - log_q_s
    sp = torch.nn.functional.softplus
    return sp(-true).sum() + sp(samp).sum()


def timed(fn, warmup, steps):
    for s in range(warmup):
        fn(s)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for s in range(steps):
        fn(warmup + s)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / max(steps, 1)


def run(shape, a):
    from openea_amd import ops
    from openea_amd.modules.base.initializers import glorot_uniform_host, xavier_host
    dev = ops.device()
    name, E, R, B = SHAPES[shape]
    d, S = a.dim, N_SAMPLED
    rng = np.random.RandomState(0)
    n_batches = a.warmup + max(a.steps, a.torch_steps + 3)
    p = 1.0 / np.arange(1, E + 1) ** 1.1
    pos = np.stack([rng.choice(E, (n_batches, B), p=p / p.sum()), rng.randint(0, R, (n_batches, B)),
                    rng.randint(0, E, (n_batches, B))], 2).astype(np.int32)
    pos_d = ops.to_ids(pos, dev)
    hosts = [xavier_host(rng, (E, d)), xavier_host(rng, (R, d)), xavier_host(rng, (E, d)), xavier_host(rng, (E,)),
             np.zeros(d, np.float32), glorot_uniform_host(rng, (d,)), glorot_uniform_host(rng, (d,)), np.zeros(d, np.float32)]

    # ---- device step ------------------------------------------------------------------------------------------------------
    v = [ops.to_table(x, dev=dev) if x.ndim == 2 else ops.to_vec(x, dev) for x in hosts]
    m, w = [torch.zeros_like(x) for x in v], [torch.zeros_like(x) for x in v]
    sampler = ops.LogUniformSampler(E, S, 7, dev)
    ws = ops.proje_workspace(E, R, d, v[0].shape[1], B, S, dev)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    ids, tries, lq = sampler.sample(0)

    def phase(ph):
        return lambda s: ops.proje_step(v, m, w, d, pos_d[s], ids, lq, tries, s + 1, 0.001, ws, loss, phase=ph, check_ids=False)

    def whole(s):
        i, t, q = sampler.sample(s)
        ops.proje_step(v, m, w, d, pos_d[s], i, q, t, s + 1, 0.001, ws, loss, check_ids=False)

    ms_sampler = timed(lambda s: sampler.sample(s), a.warmup, a.steps)
    ms_grad = timed(phase(ops.PHASE_GRAD), a.warmup, a.steps)
    ms_apply = timed(phase(ops.PHASE_APPLY), a.warmup, a.steps)
    ms_step = timed(whole, a.warmup, a.steps)
    res = dict(metric="proje_step", shape=name, dim=d, batch=B, n_sampled=S, n_ent=E, n_rel=R,
               device_ms_per_step=round(ms_step, 4), sampler_ms=round(ms_sampler, 4), grad_phase_ms=round(ms_grad, 4),
               adam_ms=round(ms_apply, 4), adam_share=round(ms_apply / ms_step, 3),
               nce_gflop_per_step=round(3 * 2.0 * B * S * d / 1e9, 3), nce_tflops_of_grad_phase=round(6.0 * B * S * d / ms_grad / 1e9, 2),
               num_tries=int(tries.item()), loss_finite=bool(np.isfinite(loss.item())))

    # ---- comparison leg: the reference's formulation composed in torch ---------------------------------------------------
    if a.torch_steps > 0:
        tv = [torch.from_numpy(np.asarray(x, np.float32)).to(dev).requires_grad_(True) for x in hosts]
        opt = torch.optim.Adam(tv, lr=0.001, eps=1e-8)
        ids_l = ids.long()
        cls = torch.arange(E, device=dev, dtype=torch.float64)
        log_q_all = torch.log(-torch.expm1(float(tries.item()) * torch.log1p(-(torch.log(cls + 2) - torch.log(cls + 1)) / np.log(E + 1.0)))).float()

        def torch_step(s):
            pl = pos_d[s].long()
            opt.zero_grad(set_to_none=True)
            lv = proje_torch_loss(tv, pl, ids_l, log_q_all[ids_l], log_q_all[pl[:, 2]])
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
