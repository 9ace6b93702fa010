"""Time of IPTransE's training step (oea_ptranse_step, csrc/ptranse_step.hip) at the EN-FR-15K-V1 and EN-FR-100K-V1 table shapes:
  (a) the fused step: margin pairs + path batch, one optimiser pass;
  (b) the same call with P = 0 (the plain margin step of oea_triple_step): (a) - (b) is the cost of the path half;
  (c) the reference's formulation composed in torch on the same GPU (whole-table l2_normalize every step as TF does, gathers of
      entity and relation rows, autograd, index_add_ into dense gradients, Adagrad on both tables) -- the comparison leg, never
      the product path.

    python tools/ptranse_step_time.py [--dim 100] [--warmup 20] [--steps 50] [--repeats 7] [--torch-steps 10] [--shapes 15K,100K]
                                      [--paths 83,B,10B] [--only fused] [--out profiles/ptranse_step_time.json]

Workload per shape: tables of the shape's size (30,000 entities / 477 relations / batch 5,000; 200,000 / 700 / 20,000), triples
with Zipf(1.1) relations and one uniform corruption each, path batches of 83 pairs (what the seeded synthetic EN-FR-15K-V1 graphs
give per step), of one batch size and of ten batch sizes, relations Zipf(1.1), weights uniform in 1..100.  The path counts of the real
datasets are not known here: the three sizes bracket them by assumption.  Timing: HIP events around `steps` consecutive steps
after `warmup`, `repeats` times, (a) and (b) alternating inside a repeat; reported: the median over the repeats and their min ..
max.  --only fused runs leg (a) alone (for a kernel trace).  Prints one JSON line per shape and path batch."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"15K": ("EN-FR-15K-V1", 30000, 477, 5000), "100K": ("EN-FR-100K-V1", 200000, 700, 20000)}
MARGIN, PATH_PARM, LR = 1.5, 0.1, 0.01


def zipf(rng, n_items, n):
    p = 1.0 / np.arange(1, n_items + 1) ** 1.1
    return rng.choice(n_items, n, p=p / p.sum())


def l2n_rows(x):
    return x * torch.rsqrt(torch.clamp((x * x).sum(1, keepdim=True), min=1e-12))


def torch_loss(ent, rel, b):
    e, r = l2n_rows(ent), l2n_rows(rel)
    pos, neg = b["pos"].long(), b["neg"].long()
    sp = ((e[pos[:, 0]] + r[pos[:, 1]] - e[pos[:, 2]]) ** 2).sum(1)
    sn = ((e[neg[:, 0]] + r[neg[:, 1]] - e[neg[:, 2]]) ** 2).sum(1)
    loss = torch.relu(sp + MARGIN - sn).sum()
    if b["paths"].shape[0]:
        p = b["paths"].long()
        base = r[p[:, 0]] + r[p[:, 1]]
        hp = ((base - r[p[:, 2]]) ** 2).sum(1) + MARGIN - ((base - r[b["neg_rel"].long()]) ** 2).sum(1)
        loss = loss + PATH_PARM * ((1.0 / b["weight"]) * torch.relu(hp)).sum()
    return loss


def stats(xs):
    return dict(median=round(float(np.median(xs)), 4), min=round(float(min(xs)), 4), max=round(float(max(xs)), 4))


def run(shape, n_paths_spec, a):
    from openea_amd import ops
    dev = ops.device()
    name, n_ent, n_rel, batch = SHAPES[shape]
    n_paths = {"B": batch, "10B": 10 * batch}.get(n_paths_spec) or int(n_paths_spec)
    d = a.dim
    rng = np.random.RandomState(0)
    tables = [(rng.standard_normal((n, d)) / np.sqrt(d)).astype(np.float32) for n in (n_ent, n_rel)]
    n_batches = 4                                                    # rotated: no step repeats its predecessor's batch

    def make_batch():
        pos = np.stack([rng.randint(0, n_ent, batch), zipf(rng, n_rel, batch), rng.randint(0, n_ent, batch)], 1).astype(np.int32)
        neg = pos.copy()
        neg[np.arange(batch), rng.randint(0, 2, batch) * 2] = rng.randint(0, n_ent, batch)
        q = np.stack([zipf(rng, n_rel, n_paths) for _ in range(4)], 1).astype(np.int32)
        return dict(pos=ops.to_ids(pos, dev), neg=ops.to_ids(neg, dev), paths=ops.to_ids(np.ascontiguousarray(q[:, :3]), dev),
                    neg_rel=ops.to_ids(np.ascontiguousarray(q[:, 3]), dev),
                    weight=ops.to_vec(rng.randint(1, 101, n_paths).astype(np.float32), dev))
    batches = [make_batch() for _ in range(n_batches)]

    def state():
        e, r = ops.to_table(tables[0], dev=dev), ops.to_table(tables[1], dev=dev)
        return dict(e=e, r=r, ea=torch.full_like(e, 0.1), ra=torch.full_like(r, 0.1),
                    cfg=ops.make_step_cfg(loss="margin-based", margin=MARGIN, optimizer="Adagrad", lr=LR),
                    ws=ops.step_workspace(n_ent, n_rel, e.shape[1], dev), pws=ops.path_workspace(n_rel, r.shape[1], dev),
                    loss=torch.zeros(1, dtype=torch.float64, device=dev))
    fused, plain = state(), state()

    def step(s, i, with_paths):
        b = batches[i % n_batches]
        ops.ptranse_step(s["e"], s["ea"], s["r"], s["ra"], d, b["pos"], b["neg"], b["paths"] if with_paths else None, b["neg_rel"],
                         b["weight"], PATH_PARM, s["cfg"], s["ws"], s["pws"], s["loss"], check_ids=False)

    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn, n):
        t0.record()
        for i in range(n):
            fn(i)
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / n
    for i in range(a.warmup):
        step(fused, i, True)
        if a.only != "fused":
            step(plain, i, False)
    ms_a, ms_b = [], []
    for _ in range(a.repeats):
        ms_a.append(timed(lambda i: step(fused, i, True), a.steps))
        if a.only != "fused":
            ms_b.append(timed(lambda i: step(plain, i, False), a.steps))
    ops.path_check(fused["pws"][1])
    res = dict(metric="ptranse_step", shape=name, dim=d, n_ent=n_ent, n_rel=n_rel, batch=batch, path_pairs=n_paths,
               fused_ms=stats(ms_a), loss_finite=bool(np.isfinite(fused["loss"].item())))
    if a.only != "fused":
        res["p0_ms"] = stats(ms_b)
        res["path_half_ms"] = round(res["fused_ms"]["median"] - res["p0_ms"]["median"], 4)
    if a.only != "fused" and a.torch_steps > 0:
        tv = [torch.from_numpy(t).to(dev).requires_grad_(True) for t in tables]
        acc = [torch.full_like(v, 0.1) for v in tv]

        def torch_step(i):
            grads = torch.autograd.grad(torch_loss(tv[0], tv[1], batches[i % n_batches]), tv)
            with torch.no_grad():
                for v, g, ac in zip(tv, grads, acc):
                    ac.addcmul_(g, g)
                    v.sub_(LR * g / ac.sqrt())
        for i in range(3):
            torch_step(i)
        ms_c = [timed(torch_step, a.torch_steps) for _ in range(min(a.repeats, 3))]
        res["torch_composed_ms"] = stats(ms_c)
        res["speedup"] = round(res["torch_composed_ms"]["median"] / res["fused_ms"]["median"], 2)
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--torch-steps", type=int, default=10)
    ap.add_argument("--shapes", default="15K,100K")
    ap.add_argument("--paths", default="83,B,10B")
    ap.add_argument("--only", default="", help="'fused': leg (a) alone")
    ap.add_argument("--out", default=None, help="also write the results as a JSON list here")
    a = ap.parse_args()
    out = [run(s, p, a) for s in a.shapes.split(",") for p in a.paths.split(",")]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
