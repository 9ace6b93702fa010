"""IMUSE without a GPU: the restatements the GPU tests (test_imuse_gpu.py) hold the kernels to -- LCS by the quadratic DP, the
ratio 2 LCS / (|a| + |b|), the bit-vector recurrence of csrc/lcs_sim.hip in Python integers, the records of run_one_ea's walk, the
alignment step in numpy -- and the host functions of approaches/imuse.py, against the fixture made from the reference's own code
(tests/golden/make_imuse_golden.py).  The fixture's ratios come from a stand-in that is this file's definition, so the ratio
itself is pinned by the literal cases below, not by the fixture."""
import hashlib
import json
import os
import random

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from openea_amd.approaches import imuse  # noqa: E402  (what this file is about: without it nothing here can run)
from openea_amd.approaches.imuse import IMUSE  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
FD_TOL = 1e-6        # central differences at 1e-6 against analytic gradients: the tolerance test_jape_cpu.py uses


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "imuse.json"), encoding="utf8") as f:
        return json.load(f)


# ---- the restatements ---------------------------------------------------------------------------------------------------------------
def dp_lcs(a, b):
    """the length of the longest common subsequence of two sequences, by rows of the quadratic table"""
    row = [0] * (len(b) + 1)
    for x in a:
        prev = 0
        for j, y in enumerate(b):
            prev, row[j + 1] = row[j + 1], (prev + 1 if x == y else max(row[j + 1], row[j]))
    return row[len(b)]


def ratio(a, b):
    """Levenshtein.ratio: (|a| + |b| - d) / (|a| + |b|) with substitutions at cost 2 = 2 LCS / (|a| + |b|); 1.0 for two empty strings"""
    return 2 * dp_lcs(a, b) / (len(a) + len(b)) if len(a) + len(b) else 1.0


def bitvector_lcs(pattern, text, word_bits=64):
    """csrc/lcs_sim.hip's recurrence with its word structure: the add carries from word to word, the subtract V - u is V & ~PM"""
    words = max(1, -(-len(pattern) // word_bits))
    full = (1 << word_bits) - 1
    pm = {}
    for p, c in enumerate(pattern):
        pm.setdefault(c, [0] * words)[p // word_bits] |= 1 << (p % word_bits)
    v = [full] * words
    for c in text:
        m, carry = pm.get(c, [0] * words), 0
        for w in range(words):
            u = v[w] & m[w]
            s = v[w] + u + carry
            carry = s >> word_bits
            v[w] = (s & full) | (v[w] & ~m[w] & full)
    return sum(bin(~x & full).count("1") for x in v)


def records_reference(strings1, strings2, idx1, idx2, threshold):
    """imuse.py:47-62 for every row: s = mean ratio over the attribute pairs both hold, in the order of k, in Python floats; a
    record where s > threshold and s > every earlier s of the row -> (ptr, col, val) as ops.attr_sim_records returns them"""
    K, n1 = idx1.shape
    n2 = idx2.shape[1]
    cache = {}
    ptr, col, val = [0], [], []
    for i in range(n1):
        sim_max = threshold
        for j in range(n2):
            sim, sim_cnt = 0, 0
            for k in range(K):
                if idx1[k, i] >= 0 and idx2[k, j] >= 0:
                    key = (int(idx1[k, i]), int(idx2[k, j]))
                    if key not in cache:
                        cache[key] = ratio(strings1[key[0]], strings2[key[1]])
                    sim += cache[key]
                    sim_cnt += 1
            if sim_cnt > 0:
                sim /= sim_cnt
            if sim > sim_max:
                sim_max = sim
                col.append(j)
                val.append(float(sim))
        ptr.append(len(col))
    return np.array(ptr, np.int64), np.array(col, np.int32), np.array(val, np.float64)


def dp_lcs_np(a, b):
    """dp_lcs with a row at a time in numpy, for the long strings of the GPU tests: cur[j] = max(prev[j], prev[j - 1] + eq_j, cur[j - 1])
    and cur is non-decreasing, so cur = the running maximum of max(prev[j], prev[j - 1] + eq_j)"""
    b = np.array([ord(c) for c in b], np.int64)
    row = np.zeros(len(b) + 1, np.int64)
    for x in a:
        row[1:] = np.maximum.accumulate(np.maximum(row[1:], row[:-1] + (b == ord(x))))
    return int(row[-1])


def ratio_table(strings1, strings2):
    """ratio of every string of one list with every string of the other -> fp64 [len1, len2], each the Python float"""
    return np.array([[(2 * dp_lcs_np(a, b) / (len(a) + len(b)) if len(a) + len(b) else 1.0) for b in strings2] for a in strings1],
                    np.float64).reshape(len(strings1), len(strings2))


def records_from_tables(table, idx1, idx2, threshold):
    """records_reference over a table of ratios (ratio_table of the two pools), whole rows at a time: numpy adds and divides
    float64 element by element in the order written, as the Python loop does"""
    K, n1 = idx1.shape
    n2 = idx2.shape[1]
    ptr, col, val = [0], [], []
    for i in range(n1):
        s, c = np.zeros(n2), np.zeros(n2, np.int64)
        for k in range(K):
            if idx1[k, i] >= 0:
                has = idx2[k] >= 0
                s = np.where(has, s + table[idx1[k, i], np.maximum(idx2[k], 0)], s)
                c += has
        s = np.where(c > 0, s / np.maximum(c, 1), s)
        before = np.maximum.accumulate(np.concatenate([[threshold], s]))[:-1]
        rec = np.flatnonzero(s > before)
        col.extend(rec.tolist())
        val.extend(s[rec].tolist())
        ptr.append(len(col))
    return np.array(ptr, np.int64), np.array(col, np.int32), np.array(val, np.float64)


def run_one_ea_from_records(ents1, ents2, ptr, col):
    """run_one_ea (imuse.py:42-66) over one chunk: the target changes at a record and is taken when nobody took it before"""
    pairs, taken = set(), set()
    for r, e1 in enumerate(ents1):
        for j in col[ptr[r]:ptr[r + 1]]:
            if ents2[j] not in taken:
                pairs.add((e1, ents2[j]))
                taken.add(ents2[j])
    return pairs


def align_loss_and_grad(ent, pairs, dt=np.float64):
    """imuse.py:304-311: loss = sum |l2n(ent)[e1] - l2n(ent)[e2]|^2 -> loss, d loss / d ent (through tf.nn.l2_normalize: x *
    rsqrt(max(sum x^2, 1e-12))), in dtype dt"""
    ent = np.asarray(ent, dt)
    inv = (1.0 / np.sqrt(np.maximum((ent * ent).sum(1, keepdims=True, dtype=dt), dt(1e-12)))).astype(dt)
    t = ent * inv
    diff = t[pairs[:, 0]] - t[pairs[:, 1]]
    g_t = np.zeros_like(t)
    np.add.at(g_t, pairs[:, 0], 2 * diff)
    np.add.at(g_t, pairs[:, 1], -2 * diff)
    grad = (g_t - t * (t * g_t).sum(1, keepdims=True, dtype=dt)) * inv
    return dt((diff * diff).sum(dtype=dt)), grad.astype(dt)


def entity_tables(golden):
    e = golden["entity"]
    tri1 = [tuple(t) for t in e["triples1"]]
    tri2 = [tuple(t) for t in e["triples2"]]
    pairs = [tuple(p) for p in e["attr_pairs"]]
    return pairs, tri1, tri2, imuse.value_tables(pairs, tri1, tri2, dev=torch.device("cpu"))


# ---- the ratio ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a, b, want", [("Hello world!", "Holly grail!", 7 / 12), ("Brian", "Jesus", 0.0), ("abc", "abd", 2 / 3),
                                        ("", "", 1.0), ("", "a", 0.0)])
def test_literal_ratios(a, b, want):
    assert ratio(a, b) == want and ratio(b, a) == want


def test_bitvector_recurrence_is_the_dp():
    rng = random.Random(5)
    for case in range(3000):
        alphabet = "ab" if case % 3 == 0 else "abcdefghijklmnopé\U0001f600"
        a = "".join(rng.choice(alphabet) for _ in range(rng.choice([0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, rng.randrange(0, 131)])))
        b = "".join(rng.choice(alphabet) for _ in range(rng.randrange(0, 90)))
        assert bitvector_lcs(a, b) == dp_lcs(a, b) == dp_lcs(b, a), (a, b)
    # small words: carries cross many word boundaries
    for _ in range(500):
        a = "".join(rng.choice("ab") for _ in range(rng.randrange(0, 40)))
        b = "".join(rng.choice("ab") for _ in range(rng.randrange(0, 40)))
        assert bitvector_lcs(a, b, word_bits=4) == dp_lcs(a, b)


def test_fast_restatements_are_the_plain_ones(golden):
    rng = random.Random(9)
    for _ in range(300):
        a = "".join(rng.choice("abcé\U0001f600") for _ in range(rng.randrange(0, 70)))
        b = "".join(rng.choice("abcé\U0001f600") for _ in range(rng.randrange(0, 70)))
        assert dp_lcs_np(a, b) == dp_lcs(a, b)
    _, _, _, (_, _, pool1, pool2, idx1, idx2) = entity_tables(golden)
    strings1, strings2 = list(pool1.index), list(pool2.index)
    table = ratio_table(strings1, strings2)
    assert table[3, 4] == ratio(strings1[3], strings2[4])
    for thr in (golden["entity"]["threshold"], 0.3, -1.0):
        plain, fast = records_reference(strings1, strings2, idx1, idx2, thr), records_from_tables(table, idx1, idx2, thr)
        assert all(np.array_equal(p, f) for p, f in zip(plain, fast)), thr           # the values bit for bit


def test_string_pool_is_utf32_code_points():
    from openea_amd import ops
    strings = ["abc", "", "héllo", "\U0001f600x\U00020000", "abc", " padded ", "Upper"]
    pool = ops.StringPool(strings, torch.device("cpu"))
    assert pool.n_str == 6 and pool.max_len == 8 and list(pool.ids(["abc", "Upper", ""])) == [0, 5, 1]
    cp, off = pool.cp.numpy(), pool.off.numpy()
    assert cp.dtype == np.int32 and off.dtype == np.int64 and off[0] == 0 and off[-1] == pool.n_cp == len(cp)
    for s, i in pool.index.items():                        # a code point per element: no surrogates, no bytes; nothing stripped
        assert [ord(c) for c in s] == list(cp[off[i]:off[i + 1]])
    empty = ops.StringPool([""], torch.device("cpu"))
    assert empty.n_str == 1 and empty.n_cp == 0 and empty.cp.numel() >= 1


# ---- the host functions against the reference's recorded outputs --------------------------------------------------------------------------
def test_filter_by_aligned_attributes_matches_the_reference(golden):
    e = golden["entity"]
    pairs, tri1, tri2, _ = entity_tables(golden)
    d1, v1 = imuse.filter_by_aligned_attributes(tri1, set(a for a, _ in pairs))
    assert list(d1.keys()) == e["filter1_entities"] and [sorted(s) for s in d1.values()] == e["filter1_attrs"]
    assert [[k[0], k[1], v] for k, v in v1.items()] == e["filter1_values"]
    d2, v2 = imuse.filter_by_aligned_attributes(tri2, set(a for _, a in pairs))
    assert list(d2.keys()) == e["filter2_entities"] and [[k[0], k[1], v] for k, v in v2.items()] == e["filter2_values"]
    twice = [t for t in tri1 if t[:2] == (144, 3)]
    assert len(twice) == 2 and v1[(144, 3)] == twice[0][2] and 109 not in d1        # the first triple of a key in the walk stays


def test_value_tables_hold_the_reference_dictionaries(golden):
    e = golden["entity"]
    pairs, _, _, (ents1, ents2, pool1, pool2, idx1, idx2) = entity_tables(golden)
    assert ents1 == e["filter1_entities"] and ents2 == e["filter2_entities"]
    assert idx1.shape == (len(pairs), len(ents1)) and idx2.shape == (len(pairs), len(ents2))
    strings1 = list(pool1.index)
    held = {(ents1[i], pairs[k][0]): strings1[idx1[k, i]] for k in range(len(pairs)) for i in range(len(ents1)) if idx1[k, i] >= 0}
    assert held == {(x[0], x[1]): x[2] for x in e["filter1_values"]}
    assert (idx2 >= 0).sum() == len(e["filter2_values"])


def test_records_and_selection_match_the_reference(golden):
    e = golden["entity"]
    _, _, _, (ents1, ents2, pool1, pool2, idx1, idx2) = entity_tables(golden)
    ptr, col, val = records_reference(list(pool1.index), list(pool2.index), idx1, idx2, e["threshold"])
    assert (np.diff(ptr) > 1).any() and (np.diff(ptr) == 0).any()
    for r in range(len(ents1)):                               # records: columns ascend, values ascend strictly above the threshold
        v = val[ptr[r]:ptr[r + 1]]
        assert (np.diff(col[ptr[r]:ptr[r + 1]]) > 0).all() and (np.diff(v) > 0).all() and (v > e["threshold"]).all()
    assert sorted(run_one_ea_from_records(ents1, ents2, ptr, col)) == [tuple(p) for p in e["run_one_ea"]]
    got = imuse.select_entity_pairs(ents1, ents2, ptr, col)
    assert sorted(got) == [tuple(p) for p in e["align_entity_by_attributes"]]
    assert len({x for x, _ in got}) == len(got)                # dict(): one pair per KG1 entity
    assert sorted(got) != [tuple(p) for p in e["run_one_ea"]]  # the eight chunks matter in this case


def test_select_entity_pairs_with_fewer_than_eight_entities():
    """size = 0: seven empty chunks and the last one with everything (imuse.py:79-86)"""
    ptr, col = np.array([0, 1, 3, 3]), np.array([2, 2, 0])
    assert imuse.select_entity_pairs([10, 11, 12], [20, 21, 22], ptr, col) == {(10, 22), (11, 20)}
    assert imuse.select_entity_pairs([], [20], np.array([0]), np.array([], np.int32)) == set()


def test_name_selection_matches_the_reference(golden):
    n = golden["names"]
    ids1, ids2 = n["ids1"], n["ids2"]
    attrs1, attrs2 = sorted(ids1.values()), sorted(ids2.values())
    name1, name2 = {i: u.split("/")[-1] for u, i in ids1.items()}, {i: u.split("/")[-1] for u, i in ids2.items()}
    sim = np.array([[ratio(name1[a], name2[b]) for b in attrs2] for a in attrs1])
    tri1, tri2 = [(e, a, "v") for e, a in n["triples1"]], [(e, a, "v") for e, a in n["triples2"]]
    for key, top_k in (("top10", 10), ("top3", 3), ("all", 99)):
        got = imuse.select_name_pairs(attrs1, attrs2, sim, n["threshold"], tri1, tri2, top_k)
        assert sorted(got) == [tuple(p) for p in n[key]], key
    got = imuse.select_name_pairs(attrs1, attrs2, sim, n["threshold"], tri1, tri2, 10)
    counts = [sum(a == a1 for _, a, _ in tri1) + sum(a == a2 for _, a, _ in tri2) for a1, a2 in got]
    assert counts == sorted(counts, reverse=True)            # a list, largest first: the order of k on the device
    taken = [b for _, b in imuse.select_name_pairs(attrs1, attrs2, sim, n["threshold"], tri1, tri2, 99)]
    assert len(set(taken)) == len(taken)
    best = {a: attrs2[int(np.argmax(sim[i]))] for i, a in enumerate(attrs1) if sim[i].max() > n["threshold"]}
    assert len(best) > len(taken)                              # somebody's best match was taken before: first come, first served


# ---- the alignment step -------------------------------------------------------------------------------------------------------------------
def test_align_restatement_matches_the_reference_graph():
    z = np.load(os.path.join(HERE, "golden", "imuse_graph.npz"))
    pairs = z["align_pairs"]
    assert np.bincount(pairs[:, 1]).max() == 2 and (pairs[:, 0] == pairs[:, 1]).any()
    loss, grad = align_loss_and_grad(z["align_var_ent_embeds"], pairs)
    assert abs(loss - z["align_loss"][0]) <= 1e-12 * abs(loss)
    assert np.abs(grad - z["align_grad_ent_embeds"]).max() <= FD_TOL
    assert np.abs(z["align_var_ent_embeds"] - z["align_lr"][0] * grad - z["align_after_ent_embeds"]).max() <= FD_TOL
    untouched = np.setdiff1d(np.arange(len(grad)), pairs.reshape(-1))
    assert len(untouched) and not grad[untouched].any()


# ---- the synthetic values -------------------------------------------------------------------------------------------------------------------
def test_default_synthetic_attributes_are_unchanged():
    """the digests of what generate_attribute_triples returned before the string option existed"""
    from openea_amd.modules.load.synth import generate_attribute_triples
    want = {"tiny": "3e64d97804a755f4420d3ce5b7b5f43fd99659270152bdfc1f53db758b7913ee",
            "small": "502e6570a681a51ad755b30f5dcb00d3d5b0bcedaa28c40c1f641350e51462a4"}
    for shape, digest in want.items():
        a, b = generate_attribute_triples(shape, 0)
        assert hashlib.sha256(repr((sorted(a), sorted(b))).encode()).hexdigest() == digest, shape


def test_synthetic_string_values():
    from openea_amd.modules.load.synth import generate_attribute_triples
    plain = generate_attribute_triples("small", 0)
    att1, att2 = generate_attribute_triples("small", 0, string_values=True)
    assert (att1, att2) == generate_attribute_triples("small", 0, string_values=True)
    for old, new in zip(plain, (att1, att2)):                      # the same entities hold the same attributes
        assert {t[:2] for t in old} == {t[:2] for t in new}
    values = [t[2] for t in att1] + [t[2] for t in att2]
    lens = np.array([len(v) for v in values])
    assert (lens == 0).sum() >= 3 and (lens > 64).sum() >= 3 and (lens > 256).sum() >= 3
    assert ((lens >= 3) & (lens <= 45)).mean() > 0.9               # 3 to 40 code points before at most five insertions
    chars = "".join(values)
    non_ascii = np.mean([ord(c) > 127 for c in chars])
    assert 0.05 < non_ascii < 0.5 and sum(ord(c) > 0xFFFF for c in chars) > 20
    # aligned entities under the attribute of the same number: the same base, a few edits -- some above 0.6 and some not
    v1 = {(t[0].split("/e")[1], t[1].split("/a")[1]): t[2] for t in att1}
    v2 = {(t[0].split("/e")[1], t[1].split("/a")[1]): t[2] for t in att2}
    shared = sorted(set(v1) & set(v2))[:400]
    r = np.array([ratio(v1[k], v2[k]) for k in shared])
    assert len(shared) == 400 and (r > 0.6).mean() > 0.5 and (r <= 0.6).sum() >= 3
    other = np.array([ratio(v1[a], v2[b]) for a, b in zip(shared, shared[7:])])
    assert (other > 0.6).mean() < 0.05


# ---- the class ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", ["15K", "100K"])
def test_default_args_match_the_shipped_files(scale):
    from openea_amd.run.default_args import get_args
    shipped = json.load(open(os.path.join(HERE, "golden", "imuse_args_%s.json" % scale)))
    ours = get_args("IMUSE", scale).__dict__
    for k, v in shipped.items():
        assert k in ours and ours[k] == v, (k, v, ours.get(k))
    assert set(ours) == set(shipped)


def _imuse(**over):
    from openea_amd.run.default_args import get_args
    m = IMUSE()
    m.set_args(get_args("IMUSE", output="/tmp/oea_imuse_cpu/", training_data="synthetic/tiny/", dataset_division="f/", **over))
    return m


@pytest.mark.parametrize("over", [dict(init="xavier"), dict(loss="limited"), dict(neg_sampling="truncated"), dict(optimizer="Adagrad"),
                                  dict(eval_metric="cosine"), dict(loss_norm="L1"), dict(ent_l2_norm=False), dict(rel_l2_norm=False),
                                  dict(neg_triple_num=2), dict(learning_rate=0.001)])
def test_init_asserts(over):
    """imuse.py:264-276, before anything is computed (no GPU here)"""
    m = _imuse(**over)
    with pytest.raises(AssertionError):
        m.init()
    assert m.ent_embeds is None and m.aligned_ent_pair_set is None


def test_more_than_one_interactive_round_is_refused():
    with pytest.raises(NotImplementedError, match="imuse.py:130-133"):
        imuse.interactive_model(None, _imuse(interactive_model_iter_num=2).args)
    m = _imuse(dim=129)
    with pytest.raises(NotImplementedError, match="129"):
        m.init()


def test_exports_and_the_reference_names():
    from openea_amd import approaches
    assert approaches.IMUSE is IMUSE
    for name in ("init", "launch_triple_training_1epo", "launch_align_training_1epo", "run", "valid", "test", "save"):
        assert callable(getattr(IMUSE, name)), name
    for name in ("interactive_model", "align_entity_by_attributes", "filter_by_aligned_attributes",
                 "get_aligned_attr_pair_by_name_similarity"):
        assert callable(getattr(imuse, name)), name
