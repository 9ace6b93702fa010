"""Times of MultiKE's device steps -- the two-net attribute step (oea_multike_cnn_step on both nets + the pull towards the names + the
engine's apply phase on both table pairs), the one-net cross-KG step, the relation view's cross-view terms and the common-space
step (oea_multike_rows + apply) -- at the attribute shapes of EN-FR-15K-V1 and EN-FR-100K-V1 (modules/load/synth.py: SHAPES,
ATTRIBUTES, what make_kgs builds) with the shipped batch sizes, each next to the reference's formulation composed in torch on the same
device (whole-table l2_normalize every step as TF does, the two convolutions as shifted-slice products -- no library convolution
call --, autograd, torch.optim.SGD): the comparison leg, never the product path.

    python tools/multike_step_time.py [--dim 100] [--warmup 10] [--steps 50] [--torch-steps 10] [--shapes 15K,100K] [--only attr]
                                      [--out FILE]

Device timing: HIP events around `steps` consecutive calls after `warmup` calls.  --only attr runs the two-net attribute step alone
(the profiler's run: tools/prof.sh trace).  Prints one JSON line per shape."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.jape_step_time import l2n, timed, zipf  # noqa: E402

LR, BN_C = 0.001, float(1.0 / np.sqrt(1.0 + 1e-3))
BATCH = {"15K": 5000, "100K": 20000}
NAMES = {"15K": "EN-FR-15K-V1", "100K": "EN-FR-100K-V1"}


def cnn_host(rng, d):
    lim = lambda fi, fo: np.sqrt(6.0 / (fi + fo))            # noqa: E731
    return [np.ones(d), np.zeros(d), rng.uniform(-lim(8, 16), lim(8, 16), (2, 4, 1, 2)), np.zeros(2),
            rng.uniform(-lim(16, 16), lim(16, 16), (2, 4, 2, 2)), np.zeros(2), rng.uniform(-lim(4 * d, d), lim(4 * d, d), (4 * d, d)),
            np.zeros(d)]


def torch_conv(x, K, b):
    """x [B, 2, d, ci] -> tanh('same' cross-correlation with K [2, 4, ci, co] + b)"""
    B, _, d, _ = x.shape
    xp = torch.nn.functional.pad(x, (0, 0, 1, 2, 0, 1))
    out = b
    for kh in range(2):
        for kw in range(4):
            out = out + xp[:, kh:kh + 2, kw:kw + d] @ K[kh, kw]
    return torch.tanh(out)


def torch_cnn_loss(p, h, a, v, w):
    x = (torch.stack([a, v], 1) * (p[0] * BN_C) + p[1]).unsqueeze(-1)
    z = torch_conv(torch_conv(x, p[2], p[3]), p[4], p[5])
    n = z * torch.rsqrt(torch.clamp((z * z).sum(2, keepdim=True), min=1e-12))
    t = torch.tanh(n.reshape(len(a), -1) @ p[6] + p[7])
    y = t * torch.rsqrt(torch.clamp((t * t).sum(), min=1e-12))
    s = torch.nn.functional.softplus(((h - y) ** 2).sum(1))
    return (s * w).sum() if w is not None else s.sum()


def run(shape, a):
    from openea_amd import ops
    from openea_amd.modules.load.synth import ATTRIBUTES, SHAPES
    name, batch = NAMES[shape], BATCH[shape]
    n_ent = 2 * SHAPES[name][0]
    n_rel = sum(SHAPES[name][1])
    (a1, a2), (t1, t2) = ATTRIBUTES[name]
    n_attr, n_lit = a1 + a2, (t1 + t2) // 2                  # about every other value is shared
    dim, dev = a.dim, ops.device()
    rng = np.random.RandomState(0)
    res = dict(metric="multike_step", shape=name, dim=dim, batch=batch, n_ent=n_ent, n_rel=n_rel, n_attr=n_attr, n_literals=n_lit)
    host = {k: rng.standard_normal((rows, dim)) / np.sqrt(dim) for k, rows in
            (("f", n_ent), ("rv", n_ent), ("av", n_ent), ("rel", n_rel), ("attr", n_attr), ("lit", n_lit), ("name", n_ent))}
    for k in ("lit", "name"):
        host[k] /= np.linalg.norm(host[k], axis=1, keepdims=True)
    T = {k: ops.to_table(h, dev=dev) for k, h in host.items()}
    ld = T["f"].shape[1]
    sets = [cnn_host(rng, dim) for _ in range(3)]
    params = [[ops.to_table(h, ld=ld, dev=dev) if i == 6 else ops.to_vec(h.reshape(-1), dev) for i, h in enumerate(s)] for s in sets]
    ws_f, ws_rv, ws_av = (ops.step_workspace(n_ent, r, ld, dev) for r in (1, n_rel, n_attr))
    dummy = torch.zeros((1, ld), device=dev)
    empty = torch.zeros((0, 3), dtype=torch.int32, device=dev)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    cfg = lambda rel_l2: ops.make_step_cfg(loss="positive", optimizer="SGD", lr=LR, ent_l2_norm=True, rel_l2_norm=rel_l2)    # noqa: E731
    cfg_f, cfg_rv, cfg_av = cfg(False), cfg(True), cfg(False)
    att_h = np.stack([zipf(rng, n_ent, batch, 0.9), zipf(rng, n_attr, batch, 1.1), rng.randint(0, n_lit, batch)], 1)
    pos_h = np.stack([zipf(rng, n_ent, batch, 0.9), zipf(rng, n_rel, batch, 1.1), zipf(rng, n_ent, batch, 0.9)], 1)
    att, pos = ops.to_ids(att_h, dev), ops.to_ids(pos_h, dev)
    ids = ops.to_ids(rng.permutation(n_ent)[:batch], dev)
    aw = ops.to_vec(rng.randint(1, 65, n_attr) / 64.0, dev)
    cws = ops.multike_cnn_workspace(dim, ld, batch, dev)
    net_av = ops.multike_net(params[0], T["av"], ws_av, n_attr, weighted=True)
    net_f = ops.multike_net(params[1], T["f"], ws_f, 1)
    net_one = ops.multike_net(params[2], T["av"], ws_av, n_attr, factor=2.0)
    heads, tails = att[:, 0].contiguous(), pos[:, 2].contiguous()
    pos_heads = pos[:, 0].contiguous()

    def apply(t, rel, c, ws):
        ops.triple_step(t, None, rel, None, dim, empty, None, c, ws, loss, phase=ops.PHASE_APPLY)

    def pull_names(items, coef):
        ops.multike_rows(ops.MULTIKE_ROWS_PULL, T["f"], ws_f, 1, T["name"], None, 1, None, dim, items, coef, loss, b_l2_norm=False)

    def attr_step(s):
        ops.multike_cnn_step([net_av, net_f], T["attr"], T["lit"], dim, att, aw, LR, cws, loss)
        pull_names(heads, 0.5)
        apply(T["av"], T["attr"], cfg_av, ws_av)
        apply(T["f"], dummy, cfg_f, ws_f)

    def one_net_step(s):
        ops.multike_cnn_step([net_one], T["attr"], T["lit"], dim, att, None, LR, cws, loss)
        apply(T["av"], T["attr"], cfg_av, ws_av)

    def cross_step(s):
        ops.multike_rows(ops.MULTIKE_ROWS_CROSS, T["f"], ws_f, 1, T["rv"], ws_rv, n_rel, T["rel"], dim, pos, 1.0, loss, rel_side=1)
        ops.multike_rows(ops.MULTIKE_ROWS_CROSS, T["rv"], ws_rv, n_rel, T["f"], ws_f, 1, T["rel"], dim, pos, 1.0, loss, rel_side=0)
        pull_names(pos_heads, 0.5)
        pull_names(tails, 0.5)
        apply(T["rv"], T["rel"], cfg_rv, ws_rv)
        apply(T["f"], dummy, cfg_f, ws_f)

    def common_step(s):
        pull_names(ids, 1.0)
        ops.multike_rows(ops.MULTIKE_ROWS_PULL, T["f"], ws_f, 1, T["rv"], ws_rv, n_rel, None, dim, ids, 1.0, loss)
        ops.multike_rows(ops.MULTIKE_ROWS_PULL, T["f"], ws_f, 1, T["av"], ws_av, n_attr, None, dim, ids, 1.0, loss)
        apply(T["f"], dummy, cfg_f, ws_f)
        apply(T["rv"], T["rel"], cfg_rv, ws_rv)
        apply(T["av"], T["attr"], cfg_av, ws_av)

    res["attr_two_net_step_ms"] = round(timed(attr_step, a.warmup, a.steps), 4)
    if a.only == "attr":
        return res
    res["attr_one_net_step_ms"] = round(timed(one_net_step, a.warmup, a.steps), 4)
    res["relation_cross_terms_ms"] = round(timed(cross_step, a.warmup, a.steps), 4)
    res["common_space_step_ms"] = round(timed(common_step, a.warmup, a.steps), 4)
    res["loss_finite"] = bool(np.isfinite(float(loss.item())))

    # ---- the reference's formulation in torch ----
    tv = {k: torch.tensor(h, dtype=torch.float32, device=dev, requires_grad=k not in ("lit", "name")) for k, h in host.items()}
    tp = [[torch.tensor(h, dtype=torch.float32, device=dev, requires_grad=True) for h in s] for s in sets]
    al, pl, il = att.long(), pos.long(), ids.long()

    def sgd(tensors):
        return torch.optim.SGD(tensors, lr=LR)
    opt_attr = sgd([tv["av"], tv["f"], tv["attr"]] + tp[0] + tp[1])
    opt_one = sgd([tv["av"], tv["attr"]] + tp[2])
    opt_cross = sgd([tv["f"], tv["rv"], tv["rel"]])
    opt_common = sgd([tv["f"], tv["rv"], tv["av"]])

    def attr_torch(s):
        opt_attr.zero_grad(set_to_none=True)
        av, f = l2n(tv["av"]), l2n(tv["f"])
        ar, vr = tv["attr"][al[:, 1]], tv["lit"][al[:, 2]]
        fh = f[al[:, 0]]
        total = torch_cnn_loss(tp[0], av[al[:, 0]], ar, vr, aw[al[:, 1]]) + torch_cnn_loss(tp[1], fh, ar, vr, None) + \
            0.5 * ((fh - tv["name"][al[:, 0]]) ** 2).sum()
        total.backward()
        opt_attr.step()

    def one_net_torch(s):
        opt_one.zero_grad(set_to_none=True)
        av = l2n(tv["av"])
        (2.0 * torch_cnn_loss(tp[2], av[al[:, 0]], tv["attr"][al[:, 1]], tv["lit"][al[:, 2]], None)).backward()
        opt_one.step()

    def cross_torch(s):
        opt_cross.zero_grad(set_to_none=True)
        f, rv, r = l2n(tv["f"]), l2n(tv["rv"]), l2n(tv["rel"])[pl[:, 1]]
        fh, ft = f[pl[:, 0]], f[pl[:, 2]]
        total = ((fh + r - rv[pl[:, 2]]) ** 2).sum() + ((rv[pl[:, 0]] + r - ft) ** 2).sum() + \
            0.5 * ((fh - tv["name"][pl[:, 0]]) ** 2).sum() + 0.5 * ((ft - tv["name"][pl[:, 2]]) ** 2).sum()
        total.backward()
        opt_cross.step()

    def common_torch(s):
        opt_common.zero_grad(set_to_none=True)
        fe = l2n(tv["f"])[il]
        total = ((fe - tv["name"][il]) ** 2).sum() + ((fe - l2n(tv["rv"])[il]) ** 2).sum() + ((fe - l2n(tv["av"])[il]) ** 2).sum()
        total.backward()
        opt_common.step()

    for key, fn in (("attr_two_net_step", attr_torch), ("attr_one_net_step", one_net_torch), ("relation_cross_terms", cross_torch),
                    ("common_space_step", common_torch)):
        res[key + "_torch_ms"] = round(timed(fn, 3, a.torch_steps), 4)
        res[key + "_speedup"] = round(res[key + "_torch_ms"] / res[key + "_ms"], 2)
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--dim", type=int, default=100)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--torch-steps", type=int, default=10)
    p.add_argument("--shapes", default="15K,100K")
    p.add_argument("--only", default=None, choices=[None, "attr"])
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
