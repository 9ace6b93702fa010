"""bench.py's plain run (the headline only) and --dump-outputs, at the EN-FR-15K-V1 shape: the result line carries the
contract's keys and no side blocks, and two runs with the same arguments write the same outputs (the same inputs; fp32
atomics may reorder the gradient sums, so the tables agree to rounding, the sampled row ids exactly)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ent_rows", "ent_embeds", "ent_adagrad_acc", "rel_embeds", "rel_adagrad_acc", "loss_sum")


def _run(tmp_path, tag):
    out = str(tmp_path / tag)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--shape", "EN-FR-15K-V1", "--steps", "12",
           "--warmup", "3", "--dump-outputs", out]
    env = dict(os.environ, OEA_BENCH_DETAIL=str(tmp_path / ("%s_detail.json" % tag)))
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    line = p.stdout.decode().strip().splitlines()[-1]
    return json.loads(line), {k: np.load(os.path.join(out, k + ".npy")) for k in NAMES}, sorted(os.listdir(out))


def test_bench_plain_run_and_dumped_outputs(tmp_path):
    c, a, files = _run(tmp_path, "a")
    assert files == sorted(k + ".npy" for k in NAMES)
    assert c["steps"] == 12 and c["warmup"] == 3 and c["repeats"] == 1 and c["value"] > 0 and c["ms_per_step"] > 0
    assert c["unit"] == "triples/s" and c["higher_is_better"] is True and c["dtype"] == "f32"
    assert c["roofline"] is None and c["cpu_baseline"] is None and "gnn" not in c["extra"] and "shape_15k" not in c["extra"]
    n_ent = c["config"]["entities"]
    assert np.array_equal(a["ent_rows"], np.arange(n_ent))          # 30,000 x 75: the whole table fits the dump
    assert a["ent_embeds"].shape == (n_ent, 75) and a["ent_embeds"].dtype == np.float32
    assert a["ent_adagrad_acc"].shape == (n_ent, 75) and a["rel_embeds"].shape == a["rel_adagrad_acc"].shape
    assert all(np.isfinite(v).all() for v in a.values()) and a["loss_sum"][0] > 0
    assert (a["ent_adagrad_acc"] > 0.1).any() and (a["ent_adagrad_acc"] >= 0.1).all()        # trained rows, untouched rows at 0.1
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    _, b, _ = _run(tmp_path, "b")
    assert np.array_equal(a["ent_rows"], b["ent_rows"])
    for k in ("ent_embeds", "ent_adagrad_acc", "rel_embeds", "rel_adagrad_acc", "loss_sum"):
        assert np.linalg.norm(a[k] - b[k]) <= 1e-3 * np.linalg.norm(b[k]), k
