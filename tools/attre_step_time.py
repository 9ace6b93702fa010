"""Times of AttrE's device pieces -- the character step (oea_attre_char_step, with the character gradient forced onto its LDS path,
at several slab counts, and onto its atomic path), the head sampler (oea_attre_sample_heads) and the joint epoch
(oea_attre_joint_epoch) -- at the attribute shapes of EN-FR-15K-V1 and EN-FR-100K-V1 with synthetic character rows, each next to the
reference's formulation composed in torch on the same device (whole-table l2_normalize every step as TF does, the composition as a
weighted sum of gathered rows, autograd, torch.optim.SGD) -- the comparison leg, never the product path.

    python tools/attre_step_time.py [--dim 100] [--warmup 10] [--steps 50] [--torch-steps 10] [--shapes 15K,100K] [--out FILE]

Workload per shape: E entities, A attributes (both KGs'), T attribute triples with a character row of their own each (literal_len 5,
C = 100 character ids under a Zipf law, as a text's letters), B positives per batch (the shipped args files), k = 1 negative,
margin-based L2 under SGD.  Device timing: HIP events around `steps` consecutive calls after `warmup` calls.  The kernels' own
durations of one step come from torch.profiler's device activity (absent where the profiler reports no kernels).  Prints one JSON
line per shape."""
import argparse
import json
import os
import re
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.jape_step_time import l2n, timed, zipf  # noqa: E402

# name, entities, attributes, attribute triples of the two KGs, positives per batch
SHAPES = {"15K": ("EN-FR-15K-V1", 27000, 308 + 404, (73121, 67167), 5000), "100K": ("EN-FR-100K-V1", 180000, 466 + 519, (497729, 426672), 20000)}
N_CHARS, LITERAL_LEN, MARGIN, LR = 100, 5, 1.5, 0.01
SLABS = (8, 32, 128, 256, 512)


def kernel_times(fn, steps):
    """{kernel name: ms per call of fn} from torch.profiler, or None"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for s in range(steps):
                fn(s)
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            t = e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total
            if t > 0:
                found = re.search(r"(\w+)(?:<[^>]*>)?\(", e.key)            # the identifier in front of the argument list
                name = found.group(1) if found else e.key.split("(")[0].strip()
                out[name] = round(out.get(name, 0.0) + t / 1000.0 / steps, 5)
        return out or None
    except Exception as e:                                   # noqa: BLE001 (a profiler that cannot start is not this tool's subject)
        print("torch.profiler unavailable: %s" % e, file=sys.stderr)
        return None


def run(shape, a):
    from openea_amd import ops
    name, n_ent, n_attr, (t1, t2), batch = SHAPES[shape]
    dim, dev = a.dim, ops.device()
    rng = np.random.RandomState(0)
    n_tri = t1 + t2
    res = dict(metric="attre_step", shape=name, dim=dim, batch=batch, n_ent=n_ent, n_attr=n_attr, n_triples=n_tri, n_chars=N_CHARS,
               literal_len=LITERAL_LEN, lds_chars=ops.attre_lds_chars(ops.pad4(dim)))
    host = [rng.standard_normal((rows, dim)) / np.sqrt(dim) for rows in (n_ent, n_attr, N_CHARS, n_ent)]
    e_ce, at, ch, e_se = (ops.to_table(h, dev=dev) for h in host)
    value_chars = ops.to_ids(zipf(rng, N_CHARS, n_tri * LITERAL_LEN).reshape(n_tri, LITERAL_LEN), dev)
    half = n_ent // 2
    b1 = int(t1 / n_tri * batch)
    pos_h = np.stack([np.concatenate([zipf(rng, half, b1, 0.9), half + zipf(rng, n_ent - half, batch - b1, 0.9)]),
                      zipf(rng, n_attr, batch, 1.1), rng.permutation(n_tri)[:batch]], 1)
    pos = ops.to_ids(pos_h, dev)
    lists = [np.arange(half, dtype=np.int32), np.arange(half, n_ent, dtype=np.int32)]
    sides = []
    for lst in lists:
        ent_pos = np.full(n_ent, -1, np.int32)
        ent_pos[lst] = np.arange(len(lst), dtype=np.int32)
        sides += [ops.to_ids(lst, dev), ops.to_ids(ent_pos, dev)]
    neg = torch.empty(batch, dtype=torch.int32, device=dev)
    cfg = ops.make_step_cfg(loss="margin-based", margin=MARGIN, optimizer="SGD", lr=LR, neg_group_k=1)
    ws = ops.step_workspace(n_ent, n_attr, e_ce.shape[1], dev)
    cws = ops.attre_char_workspace(N_CHARS, ch.shape[1], batch, dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)

    def sample(s):
        ops.attre_sample_heads(pos, b1, 1, sides[0], sides[1], sides[2], sides[3], 1, s, out=neg)
    res["sampler_ms"] = round(timed(sample, a.warmup, a.steps), 5)

    def step(path, slabs=0):
        return lambda s: ops.attre_char_step(e_ce, None, at, None, ch, None, dim, value_chars, pos, neg, True, cfg, ws, cws, err, loss,
                                             char_path=path, n_slabs=slabs)
    res["char_step_lds_ms"] = round(timed(step(ops.ATTRE_PATH_LDS), a.warmup, a.steps), 4)
    res["char_step_atomic_ms"] = round(timed(step(ops.ATTRE_PATH_ATOMIC), a.warmup, a.steps), 4)
    for n in SLABS:
        res["char_step_lds_%d_slabs_ms" % n] = round(timed(step(ops.ATTRE_PATH_LDS, n), 3, a.steps), 4)
    res["kernels_lds_ms"] = kernel_times(step(ops.ATTRE_PATH_LDS), min(a.steps, 20))
    res["kernels_atomic_ms"] = kernel_times(step(ops.ATTRE_PATH_ATOMIC), min(a.steps, 20))
    assert int(err.item()) == 0
    res["char_loss_finite"] = bool(np.isfinite(float(loss.item())))

    tv = [torch.tensor(h, dtype=torch.float32, device=dev, requires_grad=True) for h in host]
    opt = torch.optim.SGD(tv[:3], lr=LR)
    pl, nl, vl = pos.long(), neg.long(), value_chars.long()
    w = torch.tensor([sum(1.0 / m for m in range(p + 1, LITERAL_LEN + 1)) for p in range(LITERAL_LEN)], dtype=torch.float32, device=dev)

    def char_torch(s):
        opt.zero_grad(set_to_none=True)
        en, an, cn = l2n(tv[0]), l2n(tv[1]), l2n(tv[2])
        v = (cn[vl[pl[:, 2]]] * w[None, :, None]).sum(1)
        base = an[pl[:, 1]] - v
        ps, ns = ((en[pl[:, 0]] + base) ** 2).sum(1), ((en[nl] + base) ** 2).sum(1)
        torch.relu(MARGIN + ps - ns).sum().backward()
        opt.step()
    res["char_step_torch_ms"] = round(timed(char_torch, 3, a.torch_steps), 4)

    # ---- the joint epoch: ceil(E / B) steps over all entities ----
    steps = -(-n_ent // batch)
    jloss = torch.zeros(steps, dtype=torch.float64, device=dev)
    res["joint_steps"] = steps
    res["joint_epoch_ms"] = round(timed(lambda s: ops.attre_joint_epoch(e_se, None, e_ce, None, dim, True, "SGD", LR, steps, jloss),
                                        a.warmup, a.steps), 4)
    res["joint_single_steps_ms"] = round(timed(lambda s: [ops.attre_joint_epoch(e_se, None, e_ce, None, dim, True, "SGD", LR, 1, jloss)
                                                          for _ in range(steps)], 3, a.steps), 4)
    opt2 = torch.optim.SGD([tv[3], tv[0]], lr=LR)

    def joint_torch(s):
        for _ in range(steps):
            opt2.zero_grad(set_to_none=True)
            (1 - (l2n(tv[3]) * l2n(tv[0])).sum(1)).sum().backward()
            opt2.step()
    res["joint_epoch_torch_ms"] = round(timed(joint_torch, 2, a.torch_steps), 4)
    res["char_step_speedup"] = round(res["char_step_torch_ms"] / res["char_step_lds_ms"], 2)
    res["joint_epoch_speedup"] = round(res["joint_epoch_torch_ms"] / res["joint_epoch_ms"], 2)
    res["char_lds_over_atomic"] = round(res["char_step_atomic_ms"] / res["char_step_lds_ms"], 2)
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
