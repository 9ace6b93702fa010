"""Time of SEA's mapping step and mapping epoch (oea_sea_mapping_step / oea_sea_mapping_epoch) at the EN-FR-15K-V1 and
EN-FR-100K-V1 shapes, next to the reference's formulation composed in torch on the same GPU (whole-table l2_normalize every step
as TF does, four gathers, the six products, block-wide l2_normalize, autograd, TF's dense Adam on the entity table and on both
matrices) -- the comparison leg, never the product path -- and next to the triple epoch of the same model.

    python tools/sea_mapping_time.py [--dim 100] [--warmup 20] [--steps 100] [--torch-steps 20] [--epochs 5] [--shapes 15K,100K]
                                     [--out profiles/sea_mapping_time.json]

Workload per shape: a synthetic KG pair of that shape (modules/load/synth.py, alignment_module 'mapping'), the SEA class with the
shipped args of that scale; n_l = |train links| // triple_steps labelled and n_u = |test + valid links| // triple_steps unlabelled
links per step, triple_steps = ceil(triples / batch_size).  Device step timing: HIP events around `steps` consecutive steps (mapping
step + apply phase) after `warmup`; epoch timing: wall clock around launch_*_training_1epo with a device synchronisation, median of
`epochs`.  Prints one JSON line per shape."""
import argparse
import contextlib
import io
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"15K": "EN-FR-15K-V1", "100K": "EN-FR-100K-V1"}


def l2n_rows(x):
    return x * torch.rsqrt(torch.clamp((x * x).sum(1, keepdim=True), min=1e-12))


def l2n_block(x):
    return x * torch.rsqrt(torch.clamp((x * x).sum(), min=1e-12))


def torch_loss(ent, m1, m2, b, a1, a2):
    e = l2n_rows(ent)
    l1, l2, u1, u2 = e[b[0]], e[b[1]], e[b[2]], e[b[3]]
    sup = ((l2 - l2n_block(l1 @ m1)) ** 2).sum() + ((l1 - l2n_block(l2 @ m2)) ** 2).sum()
    semi = ((u1 - l2n_block(u1 @ m1 @ m2)) ** 2).sum() + ((u2 - l2n_block(u2 @ m2 @ m1)) ** 2).sum()
    return a1 * sup + a2 * semi


def run(shape, a):
    from openea_amd import ops
    from openea_amd.approaches import SEA
    from openea_amd.modules.base import initializers
    from openea_amd.modules.load.synth import make_kgs
    from openea_amd.run.default_args import get_args
    dev = ops.device()
    name = SHAPES[shape]
    kgs = make_kgs(name, mode="mapping", seed=0)
    initializers.seed(0)
    m = SEA()
    with contextlib.redirect_stdout(io.StringIO()):
        m.set_args(get_args("SEA", shape, dim=a.dim, output="/tmp/oea_sea_time/", training_data="synthetic/%s/" % name,
                            dataset_division="fold1/"))
    m.set_kgs(kgs)
    m.init()
    d = a.dim
    triples = kgs.kg1.relation_triples_num + kgs.kg2.relation_triples_num
    triple_steps = int(math.ceil(triples / m.args.batch_size))
    lab = np.asarray(kgs.train_links, np.int32)
    unl = np.asarray(list(kgs.test_links) + list(kgs.valid_links), np.int32)
    n_l, n_u = len(lab) // triple_steps, len(unl) // triple_steps
    a1, a2 = float(m.args.alpha_1), float(m.args.alpha_2)

    # ---- epochs through the class: triple epoch, mapping epoch (one C call each) -----------------------------------------
    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3
    tri, mp = [], []
    for ep in range(1, 3 + a.epochs):
        t_tri = timed(lambda: m.launch_triple_training_1epo(ep, triple_steps, None, None, None, None))
        t_map = timed(lambda: m.launch_mapping_training_1epo(ep, triple_steps))
        if ep > 2:
            tri.append(t_tri)
            mp.append(t_map)
    ms_tri, ms_map = float(np.median(tri)), float(np.median(mp))

    # ---- device step on its own -------------------------------------------------------------------------------------------
    rng = np.random.RandomState(0)
    n_batches = a.warmup + a.steps
    bl = np.stack([lab[rng.choice(len(lab), n_l, replace=False)] for _ in range(n_batches)])          # [B, n_l, 2]
    bu = np.stack([unl[rng.choice(len(unl), n_u, replace=False)] for _ in range(n_batches)])
    ids = [ops.to_ids(np.ascontiguousarray(x), dev) for x in (bl[:, :, 0], bl[:, :, 1], bu[:, :, 0], bu[:, :, 1])]
    t = m._mapping_trainer
    ent, rel = m.ent_embeds.var, m.rel_embeds.var
    ent0 = ent[:, :d].clone()
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    empty = torch.zeros((0, 3), dtype=torch.int32, device=dev)
    work = [None]

    def dev_step(s):
        t.count_steps()
        work[0] = ops.sea_mapping_step(ent, d, ids[0][s], ids[1][s], ids[2][s], ids[3][s], m.mapping_mat_1, m.mapping_mat_2,
                                       m._mapping_state, a1, a2, t.cfg, t.ws, ent.shape[0], rel.shape[0], loss, work[0])
        ops.triple_step(ent, t.ent_acc, rel, t.rel_acc, d, empty, None, t.cfg, t.ws, t.loss, phase=ops.PHASE_APPLY)

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
    from openea_amd.modules.base.initializers import orthogonal_host
    tv = [ent0.clone().requires_grad_(True)] + [torch.from_numpy(orthogonal_host(rng, (d, d))).to(dev).requires_grad_(True)
                                                 for _ in range(2)]
    tm, tvv = [torch.zeros_like(v) for v in tv], [torch.zeros_like(v) for v in tv]
    lids = [x.long() for x in ids]

    def torch_step(s, step_no):
        lv = torch_loss(tv[0], tv[1], tv[2], [x[s] for x in lids], a1, a2)
        grads = torch.autograd.grad(lv, tv)
        lr_t = 0.01 * math.sqrt(1 - 0.999 ** step_no) / (1 - 0.9 ** step_no)
        with torch.no_grad():
            for v, mm, vv, g in zip(tv, tm, tvv, grads):
                mm.mul_(0.9).add_(g, alpha=0.1)
                vv.mul_(0.999).addcmul_(g, g, value=0.001)
                v.sub_(lr_t * mm / (vv.sqrt() + 1e-8))

    ms_torch = float("nan")
    if a.torch_steps > 0:                     # (0: a kernel trace of the device path alone)
        for s in range(3):
            torch_step(s, s + 1)
        t0.record()
        for s in range(a.torch_steps):
            torch_step(3 + s, 4 + s)
        t1.record()
        torch.cuda.synchronize()
        ms_torch = t0.elapsed_time(t1) / a.torch_steps

    E, ld = ent.shape
    res = dict(metric="sea_mapping", shape=name, dim=d, n_ent=E, n_l=n_l, n_u=n_u, triple_steps=triple_steps,
               device_ms_per_step=round(ms_dev, 4), torch_composed_ms_per_step=round(ms_torch, 4),
               speedup=round(ms_torch / ms_dev, 2), mapping_epoch_ms=round(ms_map, 3), triple_epoch_ms=round(ms_tri, 3),
               mapping_share_of_epoch=round(ms_map / (ms_map + ms_tri), 3),
               dense_adam_bytes_per_step=int(E * ld * 4 * 7),          # table, m, v read + written, scratch read
               dense_adam_gbps_if_alone=round(E * ld * 4 * 7 / (ms_dev * 1e-3) / 1e9, 1),
               product_gflop_per_step=round(2.0 * d * d * 3 * (2 * n_l + 4 * n_u) / 1e9, 4),
               loss_finite=bool(np.isfinite(loss.item())))
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--torch-steps", type=int, default=20)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--shapes", default="15K,100K")
    ap.add_argument("--out", default=None, help="also write the results as a JSON list here")
    a = ap.parse_args()
    out = [run(s, a) for s in a.shapes.split(",")]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
