"""Times of JAPE's three steps -- the Attr2Vec step (oea_attr2vec_step), the triple step (oea_jape_step) and one similarity step
(oea_sample_distinct + oea_jape_sim_loss) -- at the EN-FR-15K-V1 and EN-FR-100K-V1 sharing shapes, each next to the reference's
formulation composed in torch on the same device (whole-table l2_normalize every step as TF does, autograd, torch.optim.Adagrad
with initial accumulator 0.1; the similarity step as a dense [sub_mat_size, n_ref] block times the normalised reference rows) --
the comparison leg, never the product path.

    python tools/jape_step_time.py [--dim 100] [--warmup 10] [--steps 50] [--torch-steps 10] [--shapes 15K,100K] [--out FILE]

Workload per shape: A attributes (both KGs' of SURVEY Appendix B), S = (0.9 A) // 5 candidates, B pairs / positives per batch (the
shipped args files), inputs under a Zipf law; E entities, R relations, k = 1 uniform negative; n_ref = valid + test links, a CSR
with 16 entries a row, sub_mat_size 1000.  Device timing: HIP events around `steps` consecutive calls after `warmup` calls.
`attr2vec_ms` is the single-step call on ONE fixed batch of pairs with candidates drawn beforehand: neither the batch draw nor the
candidate sampler is in it.  `attr2vec_epoch_ms_per_step` is the epoch call (oea_attr2vec_epoch over a list of 40 B pairs), which
has both: the candidates of all its steps in one launch and one oea_sample_distinct per step.  The number of launches per step
and the sum of the kernels' own durations come from torch.profiler's device activity (null where the profiler reports no
kernels): what is left of the step's time is launch latency and gaps.  Prints one JSON line per shape."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# name, attributes, pairs / positives per batch, entities, relations, reference links
SHAPES = {"15K": ("EN-FR-15K-V1", 308 + 404, 5000, 27000, 477, 12000), "100K": ("EN-FR-100K-V1", 466 + 519, 20000, 180000, 700, 80000)}
SUB_MAT, ROW_NNZ = 1000, 16


def l2n(x):
    return x * torch.rsqrt(torch.clamp((x * x).sum(1, keepdim=True), min=1e-12))


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


def kernel_sum_ms(fn, steps):
    """(kernels launched, sum of their own durations in ms) per call of fn, or (None, None)"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for s in range(steps):
                fn(s)
            torch.cuda.synchronize()
        total, count = 0.0, 0
        for e in prof.key_averages():
            t = e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total
            if t > 0:
                total, count = total + t, count + e.count
        return (round(count / steps, 2), round(total / 1000.0 / steps, 4)) if total > 0 else (None, None)
    except Exception as e:                                   # noqa: BLE001 (a profiler that cannot start is not this tool's subject)
        print("torch.profiler unavailable: %s" % e, file=sys.stderr)
        return None, None


def zipf(rng, n, size, a=1.0):
    w = 1.0 / np.arange(1, n + 1) ** a
    return rng.choice(n, size, p=w / w.sum())


def run(shape, a):
    from openea_amd import ops
    name, n_attr, batch, n_ent, n_rel, n_ref = SHAPES[shape]
    dim, dev = a.dim, ops.device()
    rng = np.random.RandomState(0)
    n_s = int(0.9 * n_attr) // 5
    res = dict(metric="jape_step", shape=name, dim=dim, batch=batch, n_attr=n_attr, n_sampled=n_s, n_ent=n_ent, n_rel=n_rel, n_ref=n_ref)

    # ---- Attr2Vec ----
    host = [rng.standard_normal((n_attr, dim)) * 0.1, rng.standard_normal((n_attr, dim)) * 0.1, np.zeros(n_attr)]
    v = [ops.to_table(host[0], dev=dev), ops.to_table(host[1], dev=dev), ops.to_vec(host[2], dev)]
    accs = [torch.full_like(t, 0.1) for t in v]
    ws = ops.attr2vec_workspace(n_attr, v[0].shape[1], n_s, dev)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    pairs = ops.to_ids(np.stack([zipf(rng, n_attr, batch), rng.randint(0, n_attr, batch)], 1), dev)
    thr = ops.log_uniform_thresholds(n_attr, dev)
    n_draw = a.warmup + a.steps
    ids, tries, logq, status = ops.log_uniform_sample_steps(n_attr, n_s, 1, 0, n_draw, thr)
    assert int(status.abs().sum()) == 0
    tries_1 = [tries[s:s + 1] for s in range(n_draw)]

    def a2v(s, phase=ops.PHASE_BOTH):
        ops.attr2vec_step(v, accs, dim, pairs, ids[s % n_draw], logq[s % n_draw], tries_1[s % n_draw], 0.01, ws, loss, phase=phase)
    res["attr2vec_ms"] = round(timed(a2v, a.warmup, a.steps), 4)
    res["attr2vec_grad_phase_ms"] = round(timed(lambda s: a2v(s, ops.PHASE_GRAD), 2, a.steps), 4)
    res["attr2vec_launches"], res["attr2vec_kernel_sum_ms"] = kernel_sum_ms(a2v, min(a.steps, 20))
    pair_list = ops.to_ids(np.stack([zipf(rng, n_attr, 40 * batch), rng.randint(0, n_attr, 40 * batch)], 1), dev)
    bufs = [None]

    def a2v_epoch(s):
        bufs[0] = ops.attr2vec_epoch(v, accs, dim, pair_list, batch, 20, 1, 20 * s, thr, n_s, 0.01, ws, loss, bufs[0])
    res["attr2vec_epoch_ms_per_step"] = round(timed(a2v_epoch, 1, 3) / 20, 4)
    assert int(bufs[0][3].count_nonzero()) == 0
    res["sampler_steps_ms_per_step"] = round(timed(lambda s: ops.log_uniform_sample_steps(n_attr, n_s, 1, 0, n_draw, thr,
                                                                                             out=(ids, tries, logq, status)), 2, 5) / n_draw, 5)
    res["attr2vec_loss_finite"] = bool(np.isfinite(float(loss.item())))
    tv = [torch.tensor(h, dtype=torch.float32, device=dev, requires_grad=True) for h in host]
    opt = torch.optim.Adagrad(tv, lr=0.01, initial_accumulator_value=0.1)
    lp = pairs.long()
    sp = torch.nn.functional.softplus
    inv_log = 1.0 / np.log(n_attr + 1.0)
    p_lab = (torch.log(lp[:, 1] + 2.0) - torch.log(lp[:, 1] + 1.0)) * inv_log

    def a2v_torch(s):
        c = ids[s % n_draw].long()
        opt.zero_grad(set_to_none=True)
        x, w = l2n(tv[0])[lp[:, 0]], l2n(tv[1])
        log_q_lab = torch.log(-torch.expm1(tries_1[s % n_draw].double() * torch.log1p(-p_lab.double()))).float()
        true = (x * w[lp[:, 1]]).sum(1) + tv[2][lp[:, 1]] - log_q_lab
        samp = x @ w[c].t() + tv[2][c] - logq[s % n_draw]
        (sp(-true) + sp(samp).sum(1)).mean().backward()
        opt.step()
    res["attr2vec_torch_ms"] = round(timed(a2v_torch, 3, a.torch_steps), 4)

    # ---- the triple step ----
    eh, rh = rng.standard_normal((n_ent, dim)) / np.sqrt(dim), rng.standard_normal((n_rel, dim)) / np.sqrt(dim)
    e, r = ops.to_table(eh, dev=dev), ops.to_table(rh, dev=dev)
    cfg = ops.make_step_cfg(loss="margin-based", optimizer="Adagrad", lr=0.01, neg_group_k=1)
    e_acc, r_acc = torch.full_like(e, 0.1), torch.full_like(r, 0.1)
    sws = ops.step_workspace(n_ent, n_rel, e.shape[1], dev)
    pos_h = np.stack([zipf(rng, n_ent, batch, 0.9), zipf(rng, n_rel, batch, 1.1), rng.randint(0, n_ent, batch)], 1)
    neg_h = pos_h.copy()
    side = rng.randint(0, 2, batch) * 2
    neg_h[np.arange(batch), side] = rng.randint(0, n_ent, batch)
    pos, neg = ops.to_ids(pos_h, dev), ops.to_ids(neg_h, dev)
    res["triple_ms"] = round(timed(lambda s: ops.jape_step(e, e_acc, r, r_acc, dim, pos, neg, 0.1, cfg, sws, loss), a.warmup, a.steps), 4)
    te = [torch.tensor(h, dtype=torch.float32, device=dev, requires_grad=True) for h in (eh, rh)]
    opt2 = torch.optim.Adagrad(te, lr=0.01, initial_accumulator_value=0.1)
    pl, nl = pos.long(), neg.long()

    def triple_torch(s):
        opt2.zero_grad(set_to_none=True)
        en, rn = l2n(te[0]), l2n(te[1])
        score = lambda t: ((en[t[:, 0]] + rn[t[:, 1]] - en[t[:, 2]]) ** 2).sum()          # noqa: E731
        (score(pl) - 0.1 * score(nl)).backward()
        opt2.step()
    res["triple_torch_ms"] = round(timed(triple_torch, 3, a.torch_steps), 4)

    # ---- one similarity step ----
    ref1, ref2 = ops.to_ids(rng.permutation(n_ent)[:n_ref], dev), ops.to_ids(rng.permutation(n_ent)[:n_ref], dev)
    indptr = torch.arange(0, (n_ref + 1) * ROW_NNZ, ROW_NNZ, dtype=torch.int64, device=dev)
    col = ops.to_ids(np.sort(rng.randint(0, n_ref, (n_ref, ROW_NNZ)), axis=1).reshape(-1), dev)
    val = ops.to_vec(0.95 + 0.05 * rng.rand(n_ref * ROW_NNZ), dev)
    idx = torch.zeros(SUB_MAT, dtype=torch.int32, device=dev)

    def sim(s):
        ops.sample_distinct(n_ref, SUB_MAT, 1, s, out=idx)
        ops.jape_sim_loss(e, dim, ref1, ref2, indptr, col, val, idx, 0.001, loss)
    res["sim_ms"] = round(timed(sim, a.warmup, a.steps), 4)
    block = torch.zeros((SUB_MAT, n_ref), dtype=torch.float32, device=dev)
    block.scatter_(1, col[:SUB_MAT * ROW_NNZ].long().reshape(SUB_MAT, ROW_NNZ), val[:SUB_MAT * ROW_NNZ].reshape(SUB_MAT, ROW_NNZ))
    r1l, r2l = ref1.long(), ref2.long()

    def sim_torch(s):
        with torch.no_grad():
            en = l2n(te[0])
            pick = torch.randperm(n_ref, device=dev)[:SUB_MAT]
            t = l2n(block @ en[r2l])
            return 0.001 * ((en[r1l[pick]] - t) ** 2).sum()
    res["sim_torch_ms"] = round(timed(sim_torch, 3, a.torch_steps), 4)
    for k in ("attr2vec", "triple", "sim"):
        res[k + "_speedup"] = round(res[k + "_torch_ms"] / res[k + "_ms"], 2)
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--dim", type=int, default=100)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--torch-steps", type=int, default=10)
    p.add_argument("--shapes", default="15K,100K")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    results = []
    for shape in a.shapes.split(","):
        results.append(run(shape, a))
        print(json.dumps(results[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
