"""IMUSE on the device: oea_lcs_ratio_pairs and oea_attr_sim_records (csrc/lcs_sim.hip) against the restatements of
test_imuse_cpu.py -- LCS lengths as integers, ratios and record values bit for bit in float64 --, the entity and the name step
against the reference's recorded outputs, what the entry points refuse, the alignment step against float64 under the tolerance
rule of tests/_grads.py, and IMUSE end to end on the tiny shape with string values."""
import functools
import json
import os
import random
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_imuse_cpu import (HERE, align_loss_and_grad, bitvector_lcs, dp_lcs_np, ratio_table, records_from_tables)  # noqa: E402

LENGTHS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000)
ALPHABETS = {
    "two letters": ("ab", "ab"),                                         # long LCS, long carry chains across the words
    "ascii": ("".join(chr(c) for c in range(32, 127)),) * 2,
    "latin with accents": ("abcdefghijklmnopqrstuvwxyzàáâãäåæçèéêëìíîïñòóôõöùúûüýÿß",) * 2,
    "above U+FFFF": ("\U0001f600\U0001f601\U00010348\U0001d11e\U00020000\U0002a6d6ab",) * 2,
    "disjoint": ("abcdefgh", "stuvwxyz"),                                # LCS 0
}


def _strings(alphabet, seed):
    rng = random.Random(seed)
    return ["".join(rng.choice(alphabet) for _ in range(n)) for n in LENGTHS]


@functools.lru_cache(maxsize=None)
def pair_case(name):
    """every length of LENGTHS on one side against every length on the other -> (strings1, strings2, pairs [256, 2], lcs [256]);
    'identical': each string against itself and against every other one of the same list"""
    if name == "identical":
        s1 = s2 = _strings(ALPHABETS["ascii"][0], 3)
    else:
        s1, s2 = _strings(ALPHABETS[name][0], 1), _strings(ALPHABETS[name][1], 2)
    pairs = np.array([(i, j) for i in range(len(LENGTHS)) for j in range(len(LENGTHS))], np.int32)
    lcs = np.array([dp_lcs_np(s1[i], s2[j]) for i, j in pairs], np.int32)
    return s1, s2, pairs, lcs


def _python_ratios(s1, s2, pairs, lcs):
    return np.array([(2 * int(x) / (len(s1[i]) + len(s2[j])) if len(s1[i]) + len(s2[j]) else 1.0) for (i, j), x in zip(pairs, lcs)], np.float64)


# ---- 1. pairs -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ALPHABETS) + ["identical"])
def test_lcs_ratio_pairs_equal_the_dp(name):
    from openea_amd import ops
    dev = ops.device()
    s1, s2, pairs, want = pair_case(name)
    pool1, pool2 = ops.StringPool(s1, dev), ops.StringPool(s2, dev)
    assert pool1.max_len == 1000 and pool1.n_str == len(LENGTHS)
    lcs, ratio = ops.lcs_ratio_pairs(pool1, pool2, ops.to_ids(pairs, dev))
    lcs, ratio = lcs.cpu().numpy(), ratio.cpu().numpy()
    bad = np.flatnonzero(lcs != want)
    assert not len(bad), [(LENGTHS[pairs[b, 0]], LENGTHS[pairs[b, 1]], int(lcs[b]), int(want[b])) for b in bad[:8]]
    assert np.array_equal(ratio.view(np.int64), _python_ratios(s1, s2, pairs, want).view(np.int64))          # bit for bit
    lens = np.array(LENGTHS)
    shorter, longer = np.minimum(lens[pairs[:, 0]], lens[pairs[:, 1]]), np.maximum(lens[pairs[:, 0]], lens[pairs[:, 1]])
    assert ((shorter <= 256) & (longer > 256)).any() and (shorter > 256).any()       # only the longer side above 256; both above
    if name == "disjoint":
        assert not want.any() and ratio[0] == 1.0 and not ratio[1:].any()            # ('', '') = 1.0, everything else 0.0
    if name == "identical":
        same = pairs[:, 0] == pairs[:, 1]
        assert np.array_equal(want[same], lens) and (ratio[same] == 1.0).all()
    if name == "two letters":
        assert (want[(shorter > 64)] > 32).all()


def test_literal_ratios_on_the_device():
    from openea_amd import ops
    dev = ops.device()
    cases = [("Hello world!", "Holly grail!", 7 / 12), ("Brian", "Jesus", 0.0), ("abc", "abd", 2 / 3), ("", "", 1.0), ("", "a", 0.0),
             ("a", "", 0.0), ("abcde", "abcxy", 0.6)]
    pool1, pool2 = ops.StringPool([c[0] for c in cases], dev), ops.StringPool([c[1] for c in cases], dev)
    pairs = np.stack([pool1.ids([c[0] for c in cases]), pool2.ids([c[1] for c in cases])], 1)
    _, ratio = ops.lcs_ratio_pairs(pool1, pool2, ops.to_ids(pairs, dev))
    assert ratio.cpu().numpy().tolist() == [c[2] for c in cases]


# ---- 2. records -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def record_pools():
    """two small pools with many equal ratios between them (ties), the exact 0.6 = 2 * 3 / 10, empty strings, values of two and of
    four words, values above 256 code points on either side and one above 512, and their table of ratios"""
    rng = random.Random(11)
    short = ["".join(rng.choice("abcdé\U0001f600") for _ in range(rng.randrange(1, 12))) for _ in range(14)]
    s1 = short + ["abcde", "", "".join(rng.choice("ab") for _ in range(100)), "".join(rng.choice("abc") for _ in range(200)),
                  "".join(rng.choice("abcd") for _ in range(300)), "".join(rng.choice("ab") for _ in range(64)),
                  "".join(rng.choice("abc") for _ in range(600))]                       # beyond the DP's register row
    s2 = short[:8] + ["".join(rng.choice("abcdé\U0001f600") for _ in range(rng.randrange(1, 12))) for _ in range(8)]
    s2 += ["abcxy", "", "".join(rng.choice("ab") for _ in range(90)), "".join(rng.choice("abcd") for _ in range(280)),
           "".join(rng.choice("abc") for _ in range(70))]
    return s1, s2, ratio_table(s1, s2)


def record_case(n1, n2, K, seed):
    s1, s2, _ = record_pools()
    rng = np.random.RandomState(seed)

    def draw(n_str, n):
        idx = rng.randint(0, 16, (K, n)).astype(np.int32)                                  # mostly the short strings
        rare = rng.rand(K, n) < 0.03
        idx[rare] = rng.randint(14, n_str, int(rare.sum()))                                 # the special and the long ones
        idx[rng.rand(K, n) < 0.35] = -1
        return idx
    idx1, idx2 = draw(len(s1), n1), draw(len(s2), n2)
    if n1 > 2:
        idx1[:, 1] = -1                                                                    # a row that lacks every attribute
        idx1[:, 2] = np.array([17, 16, 18, 20, 17, 16, 14, 15, 3, 4])[:K]                  # long values: more tables than the arena holds
    if n2 > 5:
        idx2[:, 3] = -1                                                                    # a column that lacks every attribute
        idx2[:, 5] = 19
    return idx1, idx2


@pytest.mark.parametrize("K", [1, 3, 10])
@pytest.mark.parametrize("n2", [1, 64, 257, 1000])
@pytest.mark.parametrize("n1", [1, 63, 65, 130])
def test_attr_sim_records_equal_the_restatement(n1, n2, K):
    from openea_amd import ops
    dev = ops.device()
    s1, s2, table = record_pools()
    pool1, pool2 = ops.StringPool(s1, dev), ops.StringPool(s2, dev)
    idx1, idx2 = record_case(n1, n2, K, 1000 * n1 + 10 * n2 + K)
    for thr in (0.6, 0.25):
        want = records_from_tables(table, idx1, idx2, thr)
        got = ops.attr_sim_records(pool1, pool2, ops.to_ids(idx1, dev), ops.to_ids(idx2, dev), thr, cap=2)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (n1, n2, K, thr)
        assert np.array_equal(got[2].view(np.int64), want[2].view(np.int64))                # the fp64 values bit for bit
    if n1 >= 63 and n2 >= 257:
        assert np.diff(want[0]).max() > 2                                  # cap = 2 overflowed: the wrapper ran rows again
    if n1 >= 63 and n2 == 1000 and K >= 3:
        assert (want[1] >= 256).any()                                      # a record beyond the first block of columns: the maximum was carried


def test_records_threshold_ties_and_capacity():
    """K = 1, one row 'abcdefghij'.  0.6 = 2 * 3 / 10 exactly is no record at threshold 0.6; an equal similarity later is none; four
    rising similarities with cap = 1 set the overflow flag, keep the first record, and the wrapper returns all four"""
    from openea_amd import ops
    dev = ops.device()
    pool1 = ops.StringPool(["abcde", "abcdefghij"], dev)
    cols = ["abcxy", "abcxy", "vwxyz", "abcdefg", "abcdefg", "abcdefgh", "ab", "abcdefghi", "abcdefghij", "abcdefghij"]
    pool2 = ops.StringPool(cols, dev)
    idx2 = ops.to_ids(pool2.ids(cols).reshape(1, -1), dev)
    first3, short_row = idx2[:, :3].contiguous(), ops.to_ids(np.array([[0]], np.int32), dev)
    ptr, col, val = ops.attr_sim_records(pool1, pool2, short_row, first3, 0.6)
    assert ptr.tolist() == [0, 0] and len(col) == 0                       # 'abcde' against them: 0.6, 0.6, 0.0 -- none above 0.6
    ptr, col, val = ops.attr_sim_records(pool1, pool2, short_row, first3, 0.5999999999999999)
    assert col.tolist() == [0] and val.tolist() == [0.6]                  # now the first 0.6 is a record and its twin is not
    row = ops.to_ids(np.array([[1]], np.int32), dev)
    rec_col, rec_val, rec_cnt, overflow, flag = ops.attr_sim_records_raw(pool1, pool2, row, idx2, 0.6, 1)
    assert int(flag.item()) == 0 and overflow.tolist() == [1] and rec_cnt.tolist() == [1]
    assert rec_col.tolist() == [[3]] and rec_val.tolist() == [[2 * 7 / 17]]
    ptr, col, val = ops.attr_sim_records(pool1, pool2, row, idx2, 0.6, cap=1)
    assert col.tolist() == [3, 5, 7, 8] and val.tolist() == [2 * 7 / 17, 2 * 8 / 18, 2 * 9 / 19, 1.0]      # 4 and 9 are ties


# ---- 3. the reference's recorded outputs ----------------------------------------------------------------------------------------------
def test_entity_and_name_steps_equal_the_reference():
    from openea_amd.approaches import imuse
    with open(os.path.join(HERE, "golden", "imuse.json"), encoding="utf8") as f:
        g = json.load(f)
    e = g["entity"]
    kgs = types.SimpleNamespace(kg1=types.SimpleNamespace(local_attribute_triples_list=[tuple(t) for t in e["triples1"]]),
                                kg2=types.SimpleNamespace(local_attribute_triples_list=[tuple(t) for t in e["triples2"]]))
    got = imuse.align_entity_by_attributes(kgs, [tuple(p) for p in e["attr_pairs"]], e["threshold"])
    assert sorted(got) == [tuple(p) for p in e["align_entity_by_attributes"]]
    n = g["names"]
    nkgs = types.SimpleNamespace(
        kg1=types.SimpleNamespace(attributes_id_dict=n["ids1"], attributes_set=set(n["ids1"].values()),
                                  attribute_triples_list=[(a, b, "v") for a, b in n["triples1"]]),
        kg2=types.SimpleNamespace(attributes_id_dict=n["ids2"], attributes_set=set(n["ids2"].values()),
                                  attribute_triples_list=[(a, b, "v") for a, b in n["triples2"]]))
    assert sorted(imuse.get_aligned_attr_pair_by_name_similarity(nkgs, n["threshold"])) == [tuple(p) for p in n["top10"]]
    assert sorted(imuse.get_aligned_attr_pair_by_name_similarity(nkgs, n["threshold"], top_k=3)) == [tuple(p) for p in n["top3"]]


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------
def _sentinels(dev, n_rows, cap):
    return (torch.full((n_rows, cap), -7, dtype=torch.int32, device=dev), torch.full((n_rows, cap), -7.0, dtype=torch.float64, device=dev),
            torch.full((n_rows,), -7, dtype=torch.int32, device=dev), torch.full((n_rows,), -7, dtype=torch.int32, device=dev))


def _untouched(out):
    torch.cuda.synchronize()
    return all(bool((t == -7).all()) for t in out)


def test_refusals_write_nothing():
    from openea_amd import ops
    from openea_amd._lib import OpenEAHipError
    dev = ops.device()
    pool1, pool2 = ops.StringPool(["abc", "abd", ""], dev), ops.StringPool(["abc", "xyz"], dev)
    idx1 = ops.to_ids(np.array([[0, 1, 2], [1, -1, 0]], np.int32), dev)
    idx2 = ops.to_ids(np.array([[0, 1], [1, 0]], np.int32), dev)
    ok = ops.attr_sim_records(pool1, pool2, idx1, idx2, 0.1)
    assert ok[0][-1] > 0

    def records(p1=pool1, p2=pool2, i1=idx1, i2=idx2, thr=0.1, cap=2, rows=None):
        out = _sentinels(dev, i1.shape[1] if rows is None else rows.numel(), max(cap, 1))
        return out, lambda: ops.attr_sim_records_raw(p1, p2, i1, i2, thr, cap, rows, out=out)

    # what the host sees: the status, before any launch
    empty_k = torch.zeros((0, 3), dtype=torch.int32, device=dev)
    for kw in (dict(i1=empty_k, i2=torch.zeros((0, 2), dtype=torch.int32, device=dev)),                        # K = 0
               dict(i1=torch.zeros((2, 0), dtype=torch.int32, device=dev)),                                      # n1 = 0
               dict(i2=torch.zeros((2, 0), dtype=torch.int32, device=dev)),                                      # n2 = 0
               dict(cap=0), dict(thr=float("nan")),
               dict(i1=torch.zeros((33, 3), dtype=torch.int32, device=dev), i2=torch.zeros((33, 2), dtype=torch.int32, device=dev))):
        out, call = records(**kw)
        with pytest.raises(OpenEAHipError):
            call()
        assert _untouched(out), kw
    lib = ops.lib()
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.zeros(lib.oea_lcs_workspace_ints(3), dtype=torch.int32, device=dev)
    out = (torch.full((4,), -7, dtype=torch.int32, device=dev), torch.full((4,), -7.0, dtype=torch.float64, device=dev))
    pairs = ops.to_ids(np.array([[0, 0], [1, 1], [2, 0], [0, 1]], np.int32), dev)
    for n, n_str, n_cp, max_len in ((-1, 3, 6, 3), (4, 0, 6, 3), (4, 3, -1, 3), (4, 3, 6, -1)):                  # negative lengths, no strings
        rc = lib.oea_lcs_ratio_pairs(ops._p(pool1.cp), ops._p(pool1.off), n_str, n_cp, *pool2._args(), max_len, ops._p(pairs), n,
                                     ops._p(out[0]), ops._p(out[1]), ops._p(ws), ops._p(flag), None)
        assert rc != 0 and _untouched(out) and int(flag.item()) == 0

    # what lies in device memory: the check kernels set the flag and the kernels after them write nothing
    bad_pairs = ops.to_ids(np.array([[0, 0], [3, 1], [2, 0], [0, 1]], np.int32), dev)                           # string 3 of a pool of 3
    ops.lcs_ratio_pairs(pool1, pool2, bad_pairs, out=out, err_flag=flag)
    assert _untouched(out) and int(flag.item()) == 2
    with pytest.raises(OpenEAHipError, match="index"):
        ops.lcs_check(flag)
    with pytest.raises(OpenEAHipError):
        ops.lcs_ratio_pairs(pool1, pool2, ops.to_ids(np.array([[0, -1]], np.int32), dev))
    for i1, i2, rows in ((np.array([[0, 3, 2], [1, -1, 0]]), None, None), (None, np.array([[0, 1], [-2, 0]]), None),
                         (None, None, np.array([0, 3]))):
        out, call = records(i1=idx1 if i1 is None else ops.to_ids(i1, dev), i2=idx2 if i2 is None else ops.to_ids(i2, dev),
                            rows=None if rows is None else ops.to_ids(rows, dev))
        assert int(call()[4].item()) == 2 and _untouched(out)
    broken = ops.StringPool(["abc", "abd", ""], dev)
    for off in ([0, 3, 2, 6], [1, 3, 6, 6], [0, 3, 6, 7], [0, 5, 6, 6]):               # decreasing; not from 0; not to n_cp; longer than max_len
        broken.off = torch.tensor(off, dtype=torch.int64, device=dev)
        broken.max_len = 3
        out, call = records(p1=broken)
        assert int(call()[4].item()) == 1 and _untouched(out), off
    with pytest.raises(OpenEAHipError, match="offsets"):
        ops.attr_sim_records(broken, pool2, idx1, idx2, 0.1)


# ---- 5. the alignment step ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 75, 128])
def test_align_step_against_float64(d):
    """One step at lr = 1 against the float64 restatement under tests/_grads.py's rule: every row within 4 E32 + 2^-24 |after row|,
    E32 the float32 run of the restatement against its float64 run; at d = 1 its one_column_floor with the bound of a pair
    gradient on unit rows, 2 |e1 - e2| <= 4, below the 6 it keeps for pairs (TERM_BOUND['WPair']).  A KG2 entity is in two
    pairs, a KG1 entity in two, one pair joins an entity with itself, the last 50 entities are in none."""
    import _grads as G
    from openea_amd import ops
    from openea_amd.approaches.imuse import IMUSE
    from openea_amd.models.trainer import EmbeddingTable
    dev = ops.device()
    n_ent, n_pairs = 300, 120
    rng = np.random.RandomState(100 + d)
    ent = G.f32(rng.standard_normal((n_ent, d)) * 0.3)
    left, right = rng.permutation(125)[:n_pairs], 125 + rng.permutation(125)[:n_pairs]
    right[1], left[3], right[5] = right[0], left[2], left[5]
    m = IMUSE()
    m.args = types.SimpleNamespace(learning_rate=1.0, batch_size=50)
    m.ent_embeds = EmbeddingTable(ent.astype(np.float32), True, "ent_embeds", dev)
    m.aligned_ent_pair_set = set(zip(left.tolist(), right.tolist()))
    m._define_align_graph()
    pairs = m._align_pairs.cpu().numpy().astype(np.int64)
    assert len(pairs) == n_pairs and np.bincount(pairs[:, 1]).max() == 2 and (pairs[:, 0] == pairs[:, 1]).sum() == 1
    loss64, g64 = align_loss_and_grad(ent, pairs, np.float64)
    loss32, g32 = align_loss_and_grad(ent, pairs, np.float32)
    loss = float(m.align_step().item())
    after = m.ent_embeds.var.cpu().numpy()
    assert not after[:, d:].any()
    floor = 0.0
    if d == 1:
        pos = np.stack([pairs[:, 0], np.zeros(n_pairs, np.int64), pairs[:, 1]], 1)
        floor = G.one_column_floor(dict(tables=[ent], batch=dict(pos=pos, neg=np.zeros((0, 3), np.int64)), model="WPair"), 0)
    G.gradient_check("IMUSE align step d=%d" % d, ent.astype(np.float32), np.ascontiguousarray(after[:, :d]), g64,
                     g32.astype(np.float64), floor)
    assert np.array_equal(after[250:, :d], ent.astype(np.float32)[250:])
    G.loss_check("IMUSE align step d=%d" % d, loss, dict(abs_terms=float(loss64), loss64=float(loss64), loss32=float(loss32)), d)


def test_align_epoch_without_pairs_prints_zero(capsys):
    from openea_amd import ops
    from openea_amd.approaches.imuse import IMUSE
    from openea_amd.models.trainer import EmbeddingTable
    m = IMUSE()
    m.args = types.SimpleNamespace(learning_rate=0.01, batch_size=50)
    m.ent_embeds = EmbeddingTable(np.ones((5, 4), np.float32), True, "ent_embeds", ops.device())
    m.aligned_ent_pair_set = set()
    m._define_align_graph()
    before = m.ent_embeds.var.clone()
    assert m.launch_align_training_1epo(1) == 0.0 and torch.equal(m.ent_embeds.var, before)
    assert "epoch 1, align learning loss: 0.0000" in capsys.readouterr().out


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------------------------
def _fast_records(strings1, strings2, idx1, idx2, threshold):
    """records_reference with the LCS by the bit-vector recurrence in one Python integer per pattern (held to the DP in
    test_imuse_cpu.py): the tiny shape has 160,000 entity pairs"""
    K, n1 = idx1.shape
    n2 = idx2.shape[1]
    lens2 = [len(s) for s in strings2]
    cols = [[(j, int(v)) for j, v in enumerate(idx2[k]) if v >= 0] for k in range(K)]
    ptr, col, val = [0], [], []
    for i in range(n1):
        s, c = [0.0] * n2, [0] * n2
        for k in range(K):
            if idx1[k, i] < 0:
                continue
            a = strings1[idx1[k, i]]
            for j, v in cols[k]:
                tot = len(a) + lens2[v]
                s[j] += 2 * bitvector_lcs(a, strings2[v], word_bits=max(len(a), 1)) / tot if tot else 1.0
                c[j] += 1
        sim_max = threshold
        for j in range(n2):
            x = s[j] / c[j] if c[j] else s[j]
            if x > sim_max:
                sim_max = x
                col.append(j)
                val.append(x)
        ptr.append(len(col))
    return np.array(ptr, np.int64), np.array(col, np.int32), np.array(val, np.float64)


def test_end_to_end(tmp_path, capsys):
    """the tiny shape with string values: init() finds the pair set of the restatement, two epochs run, both printed losses are
    finite, valid() returns"""
    import re
    from test_imuse_cpu import ratio
    from openea_amd.approaches import IMUSE, imuse
    from openea_amd.modules.base import initializers
    from openea_amd.modules.load.synth import make_kgs
    from openea_amd.run.default_args import get_args
    initializers.seed(20190719)
    kgs = make_kgs("tiny", mode="sharing", seed=0, attributes=True, string_values=True)
    model = IMUSE()
    model.set_args(get_args("IMUSE", output=str(tmp_path) + "/out/", training_data="synthetic/tiny/", dataset_division="fold1/", dim=32,
                            batch_size=500, max_epoch=2, start_valid=2, eval_freq=2))
    model.set_kgs(kgs)
    model.init()
    # the restatement, on the host
    attrs1, attrs2 = sorted(kgs.kg1.attributes_set), sorted(kgs.kg2.attributes_set)
    name1 = {i: u.split("/")[-1] for u, i in kgs.kg1.attributes_id_dict.items()}
    name2 = {i: u.split("/")[-1] for u, i in kgs.kg2.attributes_id_dict.items()}
    sim = np.array([[ratio(name1[a], name2[b]) for b in attrs2] for a in attrs1])
    attr_pairs = imuse.select_name_pairs(attrs1, attrs2, sim, 0.6, kgs.kg1.attribute_triples_list, kgs.kg2.attribute_triples_list)
    assert len(attr_pairs) == 10 and attr_pairs == imuse.get_aligned_attr_pair_by_name_similarity(kgs, 0.6)
    ents1, ents2, pool1, pool2, idx1, idx2 = imuse.value_tables(attr_pairs, kgs.kg1.local_attribute_triples_list,
                                                                kgs.kg2.local_attribute_triples_list, dev=torch.device("cpu"))
    ptr, col, _ = _fast_records(list(pool1.index), list(pool2.index), idx1, idx2, model.args.sim_thresholds_ent)
    want = imuse.select_entity_pairs(ents1, ents2, ptr, col)
    assert len(want) > 20 and model.aligned_ent_pair_set == want
    e0 = model.ent_embeds.var.clone()
    model.run()
    assert model.valid(model.args.stop_metric) >= 0.0
    out = capsys.readouterr().out
    triple = [float(x) for x in re.findall(r"epoch \d+, avg. triple loss: ([-\d.naninf]+),", out)]
    align = [float(x) for x in re.findall(r"epoch \d+, align learning loss: ([-\d.naninf]+),", out)]
    print(triple, align, len(want))
    assert len(triple) == 2 and len(align) == 2 and all(np.isfinite(v) for v in triple + align) and align[0] > 0
    assert "Training ends. Total time" in out and "aligned_attr_pair_set: 10" in out
    assert torch.isfinite(model.ent_embeds.var).all() and not torch.equal(model.ent_embeds.var, e0)
