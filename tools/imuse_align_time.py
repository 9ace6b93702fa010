"""Times of IMUSE's interactive model -- the name step (oea_lcs_ratio_pairs over |A1| x |A2| attribute names) and
align_entity_by_attributes (oea_attr_sim_records over n1 x n2 entities and the aligned attribute pairs, then the host selection)
-- at the EN-FR-15K-V1 and EN-FR-100K-V1 attribute shapes with the synthetic string values (modules/load/synth.py).

    python tools/imuse_align_time.py [--shapes 15K,100K] [--reps 3] [--rows 16] [--out FILE]

Device timing: HIP events around `reps` consecutive calls after one warm-up call (the name step: 20 after 3).  Per shape one
JSON line with
  name_ms, name_pairs_per_s            oea_lcs_ratio_pairs over every (attribute of KG1, attribute of KG2)
  records_ms                           one oea_attr_sim_records call over all rows at capacity 16 (check kernels included)
  records_ms_rows_le_256               the same call over the rows all of whose values have at most 256 code points: the others
                                       (rows_with_a_value_above_256) leave the bit-vector for the wave-wide DP
  string_pairs, text_chars             the (value of KG1, value of KG2) pairs that call compares: sum over the aligned attribute
                                       pairs k of holders1[k] x holders2[k]; and the text code points it walks: sum_k holders1[k] x
                                       (code points of the values KG2's entities hold for k) -- counted on the host from the tables
  string_pairs_per_s, text_chars_per_s those over records_ms
  valu_share                           text_chars x 24 / records_ms over the chip's integer VALU rate, 1024 SIMDs x 32 lanes x
                                       2.4 GHz: 24 = the VALU instructions per text character in the one-word loop of the
                                       kernel's ISA (a 64-bit add or logic op counts as what it compiles to)
  align_entity_s                       wall time of imuse.align_entity_by_attributes's parts: tables (host), records (device, with
                                       the reruns of overflowed rows and the copy back), selection (host)
  python_dp_rows_s, python_dp_extrapolated_s
                                       the reference's formulation -- Levenshtein.ratio restated as the quadratic DP in pure
                                       Python -- on `rows` sampled KG1 entities against all of KG2, and that time x n1 / rows: AN
                                       EXTRAPOLATION OF A PYTHON DP on one process, not a measurement of the reference, whose
                                       Levenshtein is C and whose walk runs in eight processes.  The sampled rows' records are
                                       compared with the device's on the way.
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"15K": "EN-FR-15K-V1", "100K": "EN-FR-100K-V1"}
VALU_PER_CHAR = 24
VALU_LANE_RATE = 1024 * 32 * 2.4e9


def dp_lcs(a, b):
    row = [0] * (len(b) + 1)
    for x in a:
        prev = 0
        for j, y in enumerate(b):
            prev, row[j + 1] = row[j + 1], (prev + 1 if x == y else max(row[j + 1], row[j]))
    return row[len(b)]


def ratio(a, b):
    return 2 * dp_lcs(a, b) / (len(a) + len(b)) if len(a) + len(b) else 1.0


def events(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def attribute_kgs(shape):
    """the attribute half of a KG pair with ids, as far as IMUSE's interactive model reads it"""
    from openea_amd.modules.load.synth import generate_attribute_triples
    sides = []
    for side, triples in enumerate(generate_attribute_triples(shape, 0, string_values=True)):
        ents = {u: i for i, u in enumerate(sorted({t[0] for t in triples}, key=lambda u: int(u.split("/e")[1])))}
        attrs = {u: 1000 * side + i for i, u in enumerate(sorted({t[1] for t in triples}, key=lambda u: int(u.split("/a")[1])))}
        ids = sorted((ents[e] + 1000000 * side, attrs[a], v) for e, a, v in triples)
        sides.append(types.SimpleNamespace(attributes_id_dict=attrs, attributes_set=set(attrs.values()), attribute_triples_list=ids,
                                           local_attribute_triples_list=ids))
    return types.SimpleNamespace(kg1=sides[0], kg2=sides[1])


def run(shape, a):
    from openea_amd import ops
    from openea_amd.approaches import imuse
    dev = ops.device()
    t = time.time()
    kgs = attribute_kgs(SHAPES[shape])
    print("%s: attribute triples with string values in %.1f s" % (shape, time.time() - t), file=sys.stderr, flush=True)
    res = dict(metric="imuse_align", shape=SHAPES[shape], n_attr=[len(kgs.kg1.attributes_set), len(kgs.kg2.attributes_set)],
               attr_triples=[len(kgs.kg1.attribute_triples_list), len(kgs.kg2.attribute_triples_list)])

    # ---- the name step ----
    attrs1, attrs2 = sorted(kgs.kg1.attributes_set), sorted(kgs.kg2.attributes_set)
    names1 = [u.split("/")[-1] for u, _ in sorted(kgs.kg1.attributes_id_dict.items(), key=lambda x: x[1])]
    names2 = [u.split("/")[-1] for u, _ in sorted(kgs.kg2.attributes_id_dict.items(), key=lambda x: x[1])]
    p1, p2 = ops.StringPool(names1, dev), ops.StringPool(names2, dev)
    pairs = ops.to_ids(np.stack(np.meshgrid(p1.ids(names1), p2.ids(names2), indexing="ij"), -1).reshape(-1, 2), dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    out = (torch.empty(pairs.shape[0], dtype=torch.int32, device=dev), torch.empty(pairs.shape[0], dtype=torch.float64, device=dev))
    res["name_ms"] = round(events(lambda: ops.lcs_ratio_pairs(p1, p2, pairs, out=out, err_flag=flag), 3, 20), 4)
    ops.lcs_check(flag)
    res["name_pairs"] = int(pairs.shape[0])
    res["name_pairs_per_s"] = float("%.4g" % (pairs.shape[0] / (res["name_ms"] * 1e-3)))
    attr_pairs = imuse.get_aligned_attr_pair_by_name_similarity(kgs, 0.6)
    res["aligned_attr_pairs"] = len(attr_pairs)

    # ---- the entity step ----
    t = time.time()
    ents1, ents2, pool1, pool2, idx1, idx2 = imuse.value_tables(attr_pairs, kgs.kg1.local_attribute_triples_list,
                                                                kgs.kg2.local_attribute_triples_list, dev)
    t_tables = time.time() - t
    holders1, holders2 = (idx1 >= 0).sum(1).astype(np.int64), (idx2 >= 0).sum(1).astype(np.int64)
    chars2 = np.array([pool2.lengths[idx2[k][idx2[k] >= 0]].sum() for k in range(len(attr_pairs))], np.int64)
    res.update(n1=len(ents1), n2=len(ents2), distinct_values=[pool1.n_str, pool2.n_str], max_len=max(pool1.max_len, pool2.max_len),
               string_pairs=int((holders1 * holders2).sum()), text_chars=int((holders1 * chars2).sum()))
    d1, d2 = ops.to_ids(idx1, dev), ops.to_ids(idx2, dev)
    res["records_ms"] = round(events(lambda: ops.attr_sim_records_raw(pool1, pool2, d1, d2, 0.6, 16, err_flag=flag), 1, a.reps), 3)
    ops.lcs_check(flag)
    sec = res["records_ms"] * 1e-3
    res["string_pairs_per_s"] = float("%.4g" % (res["string_pairs"] / sec))
    res["text_chars_per_s"] = float("%.4g" % (res["text_chars"] / sec))
    res["valu_share"] = round(res["text_chars"] * VALU_PER_CHAR / sec / VALU_LANE_RATE, 4)
    # the same call over the rows whose values all fit the bit-vector (<= 256 code points): what the wave-wide DP of the others costs
    longest = np.where(idx1 >= 0, pool1.lengths[np.maximum(idx1, 0)], 0).max(0)
    short_rows = np.flatnonzero(longest <= 256)
    res["rows_with_a_value_above_256"] = int(len(ents1) - len(short_rows))
    d_rows = ops.to_ids(short_rows, dev)
    res["records_ms_rows_le_256"] = round(events(lambda: ops.attr_sim_records_raw(pool1, pool2, d1, d2, 0.6, 16, rows=d_rows, err_flag=flag),
                                                 1, a.reps), 3)
    ops.lcs_check(flag)
    t = time.time()
    ptr, col, val = ops.attr_sim_records(pool1, pool2, d1, d2, 0.6)
    t_records = time.time() - t
    t = time.time()
    found = imuse.select_entity_pairs(ents1, ents2, ptr, col)
    res["align_entity_s"] = dict(tables=round(t_tables, 3), records=round(t_records, 3), selection=round(time.time() - t, 3))
    res.update(records=int(ptr[-1]), most_records_in_a_row=int(np.diff(ptr).max()), entity_pairs=len(found),
               true_pairs=sum(1 for x, y in found if y - x == 1000000))

    # ---- the reference's formulation on a few rows: a Python DP, extrapolated ----
    strings1, strings2 = list(pool1.index), list(pool2.index)
    rows = np.random.RandomState(0).permutation(len(ents1))[:a.rows]
    t = time.time()
    for n_done, i in enumerate(rows):
        sim_max, rec = 0.6, []
        for j in range(len(ents2)):
            sim, cnt = 0, 0
            for k in range(len(attr_pairs)):
                if idx1[k, i] >= 0 and idx2[k, j] >= 0:
                    sim += ratio(strings1[idx1[k, i]], strings2[idx2[k, j]])
                    cnt += 1
            if cnt > 0:
                sim /= cnt
            if sim > sim_max:
                sim_max = sim
                rec.append((j, sim))
        got = list(zip(col[ptr[i]:ptr[i + 1]].tolist(), val[ptr[i]:ptr[i + 1]].tolist()))
        assert got == rec, (int(i), got, rec)
        print("%s: python DP row %d of %d, %.1f s" % (shape, n_done + 1, len(rows), time.time() - t), file=sys.stderr, flush=True)
    res["python_dp_rows"] = len(rows)
    res["python_dp_rows_s"] = round(time.time() - t, 2)
    res["python_dp_extrapolated_s"] = float("%.3g" % (res["python_dp_rows_s"] * len(ents1) / max(len(rows), 1)))
    res["python_dp_note"] = "extrapolation of a pure-Python DP on one process from %d rows; not a measurement of the reference" % len(rows)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="15K,100K")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    results = []
    for shape in a.shapes.split(","):
        results.append(run(shape, a))
        print(json.dumps(results[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
