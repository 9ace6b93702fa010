"""Multi-process wiring of the model layer on ONE GPU: two ranks (gloo rendezvous on 127.0.0.1, both on
cuda:0) run the same AlignE job through BasicModel -- data-parallel step (GRAD | all-reduce | APPLY),
row-sharded validation / test (with CSLS) and row-sharded neighbour refresh -- and must reproduce the
single-process run: identical integer metrics, embeddings within fp32 summation-order noise.
(The RCCL path itself needs >1 GPU; the driver's N=2,4,8 bench exercises it.)"""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r'''
import os, sys, io, contextlib, json
import numpy as np
import torch
sys.path.insert(0, os.environ["OEA_ROOT"])
world = int(os.environ.get("WORLD_SIZE", "1"))
if world > 1:
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%s" % os.environ["OEA_PORT"],
                            rank=int(os.environ["RANK"]), world_size=world)
torch.cuda.set_device(0)
from openea_amd.approaches import AlignE, AliNet, BootEA, BootEA_RotatE, BootEA_TransH, GCN_Align, MTransE
from openea_amd.models.trans import TransD, TransH
from openea_amd.modules.load.synth import make_kgs
from openea_amd.run.default_args import get_args
from openea_amd.modules.finding.alignment import greedy_alignment
kgs = make_kgs("small", mode="swapping", seed=0)
m = AlignE()
m.set_args(get_args("AlignE", output=os.environ["OEA_OUT"] + "/out/", training_data="synthetic/small/",
                    dataset_division="fold1/", dim=32, batch_size=2000, neg_triple_num=5,
                    max_epoch=int(os.environ.get("OEA_EPOCHS", "6")), start_valid=3, eval_freq=3,
                    truncated_freq=int(os.environ.get("OEA_TRUNC_FREQ", "2")), truncated_epsilon=0.9))
m.set_kgs(kgs)
m.init()
buf = io.StringIO()
with contextlib.redirect_stdout(buf):
    m.run()
    e1, e2, _ = m._eval_test_embeddings()
    res = {}
    for csls in (0, 10):
        rest, hits1, mr, mrr = greedy_alignment(m._with_dim(e1), m._with_dim(e2), [1, 5, 10], 1, "inner", False, csls, True)
        res["csls%d" % csls] = dict(hits=[int(x) for x in greedy_alignment.last["hits_cnt"]],
                                    rank_sum=int(greedy_alignment.last["rank_sum"]), rest=sorted(rest))
    nbr = m._refresh_truncated_neighbours()[0].cpu().numpy()
if os.environ.get("OEA_ONLY_ALIGNE"):
    np.savez(os.environ["OEA_OUT"] + "/aligne_w%d_r%s.npz" % (world, os.environ.get("RANK", "0")), ent=m.ent_embeds.raw(),
             rel=m.rel_embeds.raw(), res=json.dumps(res), exchange=str(m._trainer.exchange), local=int(m._trainer.local_epochs))
    if world > 1:
        dist.barrier()
    sys.exit(0)
with contextlib.redirect_stdout(buf):
    # GCN-Align: row-sharded aggregates (one all-gather per layer, forward and backward)
    g = GCN_Align()
    g.set_args(get_args("GCN_Align", output=os.environ["OEA_OUT"] + "/out/", training_data="synthetic/small/",
                        dataset_division="fold1/", max_epoch=4, start_valid=100, eval_freq=100, se_dim=32, ae_dim=16))
    g.set_kgs(make_kgs("small", mode="mapping", seed=0))
    g.init()
    g.run()
    gcn_out = g.model_se.forward()[2].cpu().numpy()
    # sparse attention operator: segments / columns sharded over the ranks (forward + backward)
    from openea_amd.models.graph_ops import EdgeGraph, sparse_attention
    from openea_amd import ops
    rng = np.random.RandomState(11)
    n, nnz, d = 700, 9000, 40
    er = np.minimum(rng.zipf(1.5, nnz) - 1, n - 1)
    graph = EdgeGraph(er, rng.randint(0, n, nnz), rng.rand(nnz).astype(np.float32), (n, n), ops.device())
    z = torch.from_numpy(rng.standard_normal(graph.nnz).astype(np.float32)).cuda().requires_grad_(True)
    v = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).cuda().requires_grad_(True)
    up = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).cuda()
    att = sparse_attention(graph, z, v)
    (att * up).sum().backward()
    attn_res = [att.detach().cpu().numpy(), z.grad.cpu().numpy(), v.grad.cpu().numpy()]
    assert (graph.shard is not None) == (world > 1)
    # the same in the AS-FED edge order with TF1's run grouping (AliNet's default): several segments per output row
    graph_r = EdgeGraph(er, rng.randint(0, n, nnz), rng.rand(nnz).astype(np.float32), (n, n), ops.device(), grouping="runs")
    zr = torch.from_numpy(rng.standard_normal(graph_r.nnz).astype(np.float32)).cuda().requires_grad_(True)
    vr = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).cuda().requires_grad_(True)
    att_r = sparse_attention(graph_r, zr, vr)
    (att_r * up).sum().backward()
    attn_res += [att_r.detach().cpu().numpy(), zr.grad.cpu().numpy(), vr.grad.cpu().numpy()]
    assert (graph_r.shard is not None) == (world > 1) and not graph_r.unique_rows
    # AliNet end to end: sharded aggregates + sharded attention inside the autograd graph, device negative sampler
    a = AliNet()
    a.set_args(get_args("AliNet", output=os.environ["OEA_OUT"] + "/out/", training_data="synthetic/small/", dataset_division="f/",
                        layer_dims=[48, 32, 24], batch_size=600, max_epoch=4, start_valid=100, eval_freq=100, truncated_epsilon=0.9))
    a.set_kgs(make_kgs("small", mode="mapping", seed=0))
    a.init()
    with torch.no_grad():
        alinet_fwd0 = a._forward()[-1].detach().cpu().numpy()           # before any step: the forward alone, sharded vs not
    # one backward on the initial parameters (the sampler state is put back afterwards): gradient by gradient, sharded vs not
    import random as _random
    _st, _pst = a._rng.get_state(), _random.getstate()
    _pos, _neg, _valid = a.device_input_batch(a.args.batch_size)
    _hs, _, _ts = a.generate_rel_batch()
    _outs = a._forward()
    _emb = a._concat_train(_outs)
    _loss = a.compute_loss(_emb, _pos, _neg, _valid) + a.compute_rel_loss(_emb, torch.as_tensor(_hs, device=a.dev), torch.as_tensor(_ts, device=a.dev))
    _loss.backward()
    alinet_grads = {"alinet_g%02d" % i: (torch.zeros_like(p) if p.grad is None else p.grad).detach().cpu().numpy() for i, p in enumerate(a._params)}
    alinet_grads.update(alinet_in_neg=_neg.cpu().numpy(), alinet_in_valid=_valid.cpu().numpy(), alinet_in_pos=np.asarray(_pos.cpu() if hasattr(_pos, "cpu") else _pos),
                        alinet_in_hs=np.asarray(_hs), alinet_in_ts=np.asarray(_ts), alinet_in_loss=np.asarray(float(_loss.detach())),
                        alinet_in_emb=_emb.detach().cpu().numpy())
    for p in a._params:
        p.grad = None
    a._rng.set_state(_st)
    _random.setstate(_pst)
    a._neg_step -= 1
    a.args.max_epoch = 1
    a.run()
    alinet_ep1 = a._forward()[-1].detach().cpu().numpy()
    a.args.max_epoch = 3
    a.run()
    alinet_out = a._forward()[-1].detach().cpu().numpy()
    # replicated small steps (MTransE mapping step, BootEA alignment step) must keep the replicas in lock-step
    extra = {}
    for cls, nm, mode, kw in ((MTransE, "MTransE", "mapping", dict(max_epoch=4, start_valid=100, eval_freq=100)),
                              (BootEA, "BootEA", "swapping", dict(max_epoch=4, sub_epoch=2, start_valid=100, sim_th=0.3)),
                              (TransD, "TransD", "sharing", dict(max_epoch=4, start_valid=100, eval_freq=100)),
                              (TransH, "TransH", "sharing", dict(max_epoch=4, start_valid=100, eval_freq=100)),
                              (BootEA_TransH, "BootEA_TransH", "swapping", dict(max_epoch=4, sub_epoch=2, start_valid=100, sim_th=0.3)),
                              (BootEA_RotatE, "BootEA_RotatE", "swapping", dict(max_epoch=4, sub_epoch=2, start_valid=100, start_bp=2,
                                                                                sim_th=0.3, gamma=6.0, neg_triple_num=4))):
        b = cls()
        b.set_args(get_args(nm, output=os.environ["OEA_OUT"] + "/out/", training_data="synthetic/small/", dataset_division="f/",
                            dim=32, batch_size=2000, **kw))
        b.set_kgs(make_kgs("small", mode=mode, seed=0))
        b.init()
        b.run()
        extra[nm] = b.ent_embeds.raw() if hasattr(b.ent_embeds, "raw") else b.ent_embeds.var.cpu().numpy()
rank = int(os.environ.get("RANK", "0"))
np.savez(os.environ["OEA_OUT"] + "/result_w%d_r%d.npz" % (world, rank), ent=m.ent_embeds.raw(), rel=m.rel_embeds.raw(),
         nbr=nbr, res=json.dumps(res), gcn_out=gcn_out, att=attn_res[0], att_dz=attn_res[1], att_dv=attn_res[2], att_r=attn_res[3], att_r_dz=attn_res[4], att_r_dv=attn_res[5], alinet=alinet_out, alinet_fwd0=alinet_fwd0, alinet_ep1=alinet_ep1, **alinet_grads, mtranse=extra["MTransE"], bootea=extra["BootEA"], transd=extra["TransD"],
         rotate=extra["BootEA_RotatE"], transh=extra["TransH"], bootea_transh=extra["BootEA_TransH"])
if world > 1:
    dist.barrier()
'''


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _launch(tmp_path, world, prefix="result", **extra_env):
    env = dict(os.environ, OEA_ROOT=ROOT, OEA_OUT=str(tmp_path), OEA_PORT=str(_free_port()), WORLD_SIZE=str(world), **extra_env)
    procs = []
    for r in range(world):
        procs.append(subprocess.Popen([sys.executable, "-c", WORKER], env=dict(env, RANK=str(r)),
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=420)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(out.decode(errors="replace"))
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    # read eagerly: a later launch with the same world size overwrites the files
    return [dict(np.load(os.path.join(str(tmp_path), "%s_w%d_r%d.npz" % (prefix, world, r))).items()) for r in range(world)]


def test_two_ranks_reproduce_single_process(tmp_path, capsys):
    import json
    single = _launch(tmp_path, 1)[0]
    r0, r1 = _launch(tmp_path, 2)
    # replicas stay bit-identical (same all-reduced gradients, same update on every rank)
    assert np.array_equal(r0["ent"], r1["ent"]) and np.array_equal(r0["rel"], r1["rel"])
    assert str(r0["res"]) == str(r1["res"]) and np.array_equal(r0["nbr"], r1["nbr"])
    # and equal the single-process job up to the order of the fp32 gradient sums
    # (6 epochs with a neighbour refresh in between amplify the 1e-7 per-step reordering noise; the per-step
    #  equivalence at 1e-4 is tests/test_dist_cpu.py::test_data_parallel_exchange_equals_big_batch)
    assert np.linalg.norm(r0["ent"] - single["ent"]) <= 5e-4 * np.linalg.norm(single["ent"])
    assert np.linalg.norm(r0["rel"] - single["rel"]) <= 5e-4 * np.linalg.norm(single["rel"])
    a, b = json.loads(str(r0["res"])), json.loads(str(single["res"]))
    for key in ("csls0", "csls10"):
        # integer metrics: sharded evaluation of (almost) the same embeddings; allow the few ranks an
        # embedding difference of 1e-4 can flip
        assert np.abs(np.array(a[key]["hits"]) - np.array(b[key]["hits"])).max() <= 3
        assert abs(a[key]["rank_sum"] - b[key]["rank_sum"]) <= 0.01 * b[key]["rank_sum"] + 3
    assert (r0["nbr"] == single["nbr"]).mean() > 0.98
    # sharded GCN aggregates: same rows computed by the same code; only hub-row atomics may reorder
    assert np.array_equal(r0["gcn_out"], r1["gcn_out"])
    np.testing.assert_allclose(r0["gcn_out"], single["gcn_out"], rtol=1e-4, atol=1e-5)
    # sharded sparse attention ('row' and 'runs' grouping): the same per-segment / per-row / per-column code on the same
    # data in the same fixed summation order (no atomics since round 3) -> the SAME BITS as the single-process operator
    for key in ("att", "att_dz", "att_dv", "att_r", "att_r_dz", "att_r_dv"):
        assert np.array_equal(r0[key], r1[key])                       # all-gathered results: identical on every rank
        assert np.array_equal(r0[key], single[key]), key
    assert np.array_equal(r0["alinet"], r1["alinet"])                  # replicas stay in lock-step through 4 Adam epochs
    def rel(key):
        return float(np.linalg.norm(r0[key] - single[key]) / np.linalg.norm(single[key]))
    d_alinet = rel("alinet")
    with capsys.disabled():
        print("\nAliNet two ranks vs single process: forward before training %.2e, after 1 Adam epoch %.2e, after 4 epochs %.2e "
              "(relative L2); GCN-Align outputs max abs %.2e"
              % (rel("alinet_fwd0"), rel("alinet_ep1"), d_alinet, float(np.abs(r0["gcn_out"] - single["gcn_out"]).max())))
        for key in sorted(k for k in single if k.startswith("alinet_in_")):
            if not np.array_equal(r0[key], single[key]):
                print("   first batch %s: sharded vs single DIFFER (%d entries)" % (key, int((r0[key] != single[key]).sum())))
        for key in sorted(k for k in single if k.startswith("alinet_g")):
            if not np.array_equal(r0[key], single[key]):
                print("   gradient %s %s: sharded vs single max abs %.2e (|g| max %.2e), differing entries %d"
                      % (key, single[key].shape, float(np.abs(r0[key] - single[key]).max()), float(np.abs(single[key]).max()),
                         int((r0[key] != single[key]).sum())))
    # round 3: bit-identical (0.00e+00) since the sparse operators have no atomics, the weight gradients a fixed summation order
    # and AliNet's triple list a canonical order (it was list(set): the relation batches followed PYTHONHASHSEED)
    assert d_alinet <= float(os.environ.get("OEA_ALINET_2RANK_TOL", "1e-6"))
    for key in ("mtranse", "bootea", "transd", "rotate", "transh", "bootea_transh"):
        assert np.array_equal(r0[key], r1[key])
        assert np.linalg.norm(r0[key] - single[key]) <= 1e-3 * np.linalg.norm(single[key])
    with capsys.disabled():
        print("two ranks vs single process, relative L2 of the entity tables: " + ", ".join(
            "%s %.2e" % (key, float(np.linalg.norm(r0[key] - single[key]) / np.linalg.norm(single[key])))
            for key in ("mtranse", "bootea", "transd", "rotate", "transh", "bootea_transh"))
              + "  (round 3: TransD's stacked tables and TransH's entity / relation tables partitioned by row id, the normal vectors replicated)")
    assert single["rotate"].dtype == np.float64


def test_epoch_exchange_replicas_agree_and_drift_is_small(tmp_path, capsys):
    """dp_exchange = 'epoch' (BASELINE.json north_star: local steps, one exchange per epoch): two ranks train their halves
    of every batch on local tables through the fused epoch call and sum the changes at the epoch's end.  The replicas must
    hold identical bits after every exchange; against the single-process job the tables DRIFT (local SGD reads rows with a
    delay of up to one epoch) -- the test prints the drift and bounds it."""
    import json
    kw = dict(OEA_ONLY_ALIGNE="1", OEA_EPOCHS="6", OEA_TRUNC_FREQ="2")
    single = _launch(tmp_path, 1, "aligne", **kw)[0]
    step = _launch(tmp_path, 2, "aligne", OEA_DP_EXCHANGE="step", **kw)[0]
    r0, r1 = _launch(tmp_path, 2, "aligne", OEA_DP_EXCHANGE="epoch", **kw)
    assert str(r0["exchange"]) == "epoch" and int(r0["local"]) == 1 and str(step["exchange"]) == "step"
    assert np.array_equal(r0["ent"], r1["ent"]) and np.array_equal(r0["rel"], r1["rel"]) and str(r0["res"]) == str(r1["res"])

    def rel(a, b):
        return float(np.linalg.norm(a - b) / np.linalg.norm(b))
    d_step, d_epoch = rel(step["ent"], single["ent"]), rel(r0["ent"], single["ent"])
    moved = rel(single["ent"], np.zeros_like(single["ent"]) + single["ent"].mean())         # scale only
    a, b = json.loads(str(r0["res"])), json.loads(str(single["res"]))
    with capsys.disabled():
        print("\nentity table after 6 epochs vs the single-process job: per-step exchange %.2e, per-epoch exchange %.2e (relative L2); "
              "hits@1 %d vs %d of %d pairs, rank sum %d vs %d" % (d_step, d_epoch, a["csls0"]["hits"][0], b["csls0"]["hits"][0],
                                                                   len(a["csls0"]["rest"]), a["csls0"]["rank_sum"], b["csls0"]["rank_sum"]))
    assert d_step <= 5e-4
    assert d_epoch <= 0.2 and moved > 0                       # same training run to first order; NOT the same bits
    assert abs(a["csls0"]["rank_sum"] - b["csls0"]["rank_sum"]) <= 0.15 * b["csls0"]["rank_sum"] + 10


@pytest.mark.parametrize("launcher", ["self", "torchrun"])
def test_bench_two_ranks_like_the_driver(tmp_path, launcher):
    """`python bench.py --gpus 2` (bench.py starts its own ranks) and `python -m torch.distributed.run --nproc-per-node 2
    bench.py --gpus 2 ...` (the driver's documented launch line), both ranks on GPU 0 with gloo collectives
    (OEA_BENCH_ONE_GPU / OEA_BENCH_BACKEND, bench.py's test hooks): the partitioned step and the row-sharded eval /
    neighbour legs run through the timed regions and rank 0 prints one well-formed line."""
    import json
    detail = str(tmp_path / "detail.json")
    env = dict(os.environ, OEA_BENCH_ONE_GPU="1", OEA_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", OEA_BENCH_DETAIL=detail)
    env.pop("WORLD_SIZE", None)
    # the default at every N is the EN-FR-100K-V1 shape; with both ranks on one GPU and the collectives staged through the host the
    # test takes the 15K shape (same code path: strong scaling, per-step partition exchange from one C call per epoch)
    tail = [os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "10", "--warmup", "3", "--repeats", "3", "--shape", "EN-FR-15K-V1",
            "--full"]
    if launcher == "self":
        cmd = [sys.executable] + tail
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
               "--master-port", str(_free_port())] + tail
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout.decode()[-2000:]
    assert lines[0] == p.stdout.decode().strip().splitlines()[-1] and len(lines[0]) < 4096      # the compact line is the LAST line
    c = json.loads(lines[0])
    assert c["n_gpus"] == 2 and c["steps"] == 10 and c["warmup"] == 3 and c["scaling"] == "strong" and c["value"] > 0
    assert 0 < c["roofline"]["frac"] <= 1 and c["roofline"]["avg_kernel_us"] > 0 and c["extra"]["exchange_mode"] == "halo"
    assert c["extra"]["exchange_phases"]["steps_timed"] == 10 and c["extra"]["single_gpu_same_config"]["value"] > 0
    assert c["extra"]["collective_world_size"] == 2 and c["extra"]["eval_pairs_per_s_inner"] > 0
    j = json.load(open(detail))                 # everything measured: bench_detail.json
    assert j["value"] == c["value"] and j["roofline"]["frac"] == c["roofline"]["frac"]
    assert j["roofline"]["launches_timed"] > 0 and j["roofline"]["avg_kernel_us"] > 0 and j["roofline"]["apply_rows_avg_us"] > 0
    assert 0 < j["roofline"]["frac"] <= 1 and 0 < j["roofline"]["frac_sec8d"] <= 1
    x = j["extra"]
    assert x["exchange_bytes_per_step_per_rank"] > 0 and x["collective_world_size"] == 2 and x["exchange_mode"] == "halo"
    assert x["exchange_bytes_per_step_per_rank"] < x["other_exchange"]["exchange_bytes_per_step_per_rank"]      # boundary rows < every owned row
    assert x["eval_pairs_per_s_inner"] > 0 and x["neighbour_rows_per_s"] > 0
    assert j["config"]["parallelism"].startswith("dp2") and j["config"]["global_batch"] == 5000       # BASELINE config 2's batch, kept global
    ph = x["exchange_phases"]                  # HIP events of the one-call partitioned epoch
    assert ph["steps_timed"] == 10 and all(ph[k + "_us"] >= 0 for k in ("grad", "pack", "reduce_scatter", "apply", "all_gather", "unpack"))
    assert ph["grad_us"] > 0 and ph["apply_us"] > 0
    assert x["single_gpu_same_config"]["value"] > 0 and x["speedup_vs_single_gpu_same_config"] > 0
    assert x["other_exchange"]["exchange_mode"] == "step" and x["local_sgd"]["exchange_mode"] == "epoch" and "parity" in x["local_sgd"]
