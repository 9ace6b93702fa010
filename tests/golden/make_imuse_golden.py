"""Recorded inputs and outputs of IMUSE's host functions and of its align_loss graph, from the REFERENCE's own code
(approaches/imuse.py: filter_by_aligned_attributes, run_one_ea, align_entity_by_attributes with its real eight-process pool,
get_aligned_attr_pair_by_name_similarity, and IMUSE._define_variables / _define_embed_graph), run unmodified through the helpers
of make_tf_graph_golden.py.  Two stand-ins sit in sys.modules: tests/golden/tf_shim.py for `tensorflow`, and a `Levenshtein`
module whose ratio is the definition 2 LCS(a, b) / (|a| + |b|) by the quadratic DP (python-Levenshtein is not installed).  So the
RATIO is ours and is not pinned by this fixture -- literal cases pin it (tests/test_imuse_cpu.py); what the fixture pins is what the
reference does WITH the ratios: which value an entity holds, the walk, the target bookkeeping, the chunks, the union, the dict.

The reference iterates sets; to give it an order, every collection handed to it here is a list (attribute triples sorted, the
aligned attribute pairs in a fixed order) or a set of small ints, which Python walks in ascending order.

Run in the build container only:  python tests/golden/make_imuse_golden.py   -> tests/golden/imuse.json, tests/golden/imuse_graph.npz
"""
import importlib
import json
import os
import random
import sys
import types

import numpy as np

from make_tf_graph_golden import HERE, fd_gradients, import_reference, quiet

ALPHABET = "abcdefghij" * 3 + "ABC -.'" + "éüñ中文\U0001f600\U00010348"


def lcs(a, b):
    row = [0] * (len(b) + 1)
    for x in a:
        prev = 0
        for j, y in enumerate(b):
            prev, row[j + 1] = row[j + 1], (prev + 1 if x == y else max(row[j + 1], row[j]))
    return row[len(b)]


def ratio(a, b):
    return 2 * lcs(a, b) / (len(a) + len(b)) if len(a) + len(b) else 1.0


def _edited(rng, chars, n_edits):
    chars = list(chars)
    for _ in range(n_edits):
        at, what, c = rng.randrange(len(chars) + 1), rng.randrange(3), rng.choice(ALPHABET)
        if what == 0 or not chars:
            chars.insert(at, c)
        elif what == 1:
            chars[min(at, len(chars) - 1)] = c
        else:
            del chars[min(at, len(chars) - 1)]
    return "".join(chars)


def entity_case(rng):
    """44 + 8 entities of KG1 against 50 of KG2 under four aligned attribute pairs.  KG1 entity 100 + i and KG2 entity 200 + i share
    a base string per attribute, each edited 0 to 4 times: at 0.6 some are found and some are not.  KG1 entities 144 .. 151 hold
    the values of 100 .. 107 again (edited once more), so entities of the first chunk and of the last want the same targets; KG2
    entities 200 .. 209 are rough copies of 230 .. 239, so a KG1 entity meets a fair match before its best one; a few entities
    lack some or all attributes; one value is empty on both sides; a second triple of one (entity, attribute) must be ignored."""
    attr_pairs = [(3, 13), (1, 11), (4, 14), (2, 12)]                    # NOT sorted: the order is the caller's
    base = {(i, k): "".join(rng.choice(ALPHABET) for _ in range(rng.randrange(3, 22))) for i in range(50) for k in range(4)}
    base[(5, 1)] = ""
    tri1, tri2 = [], []
    for i in range(44):
        for k, (a1, _) in enumerate(attr_pairs):
            if rng.random() < 0.8 and i != 9:                            # entity 109 holds none of the aligned attributes
                tri1.append((100 + i, a1, base[(i, k)] if (i, k) == (5, 1) else _edited(rng, base[(i, k)], rng.randrange(5))))
        tri1.append((100 + i, 7, "not aligned"))
    for i in range(8):
        for k, (a1, _) in enumerate(attr_pairs):
            tri1.append((144 + i, a1, _edited(rng, base[(i, k)], 1)))
    for i in range(50):
        for k, (_, a2) in enumerate(attr_pairs):
            if i < 10 and i != 5:        # a rougher copy of entity 30 + i, met first: 130 + i has two records and takes both targets
                tri2.append((200 + i, a2, _edited(rng, base[(30 + i, k)], rng.randrange(2, 5))))
            elif rng.random() < 0.85 and i != 17:
                tri2.append((200 + i, a2, base[(i, k)] if (i, k) == (5, 1) else _edited(rng, base[(i, k)], rng.randrange(4))))
    tri1.append((144, 3, "zzzz another value of a key that has one"))
    return attr_pairs, sorted(tri1), sorted(tri2)


def name_case():
    """attribute URIs of two KGs (ids ascending in each), their triples as (entity, attribute, value) with counts that differ"""
    names1 = ["http://a.org/ontology/birthDate", "http://a.org/ontology/name", "http://a.org/ontology/populationTotal",
              "http://a.org/ontology/areaCode", "http://a.org/ontology/height", "http://a.org/ontology/motto",
              "http://a.org/ontology/birthPlace", "http://a.org/ontology/elevation", "http://a.org/ontology/abbreviation",
              "http://a.org/ontology/foundingDate", "http://a.org/ontology/length", "http://a.org/ontology/weight",
              "http://a.org/ontology/isbn"]
    names2 = ["http://b.org/prop/dateDeNaissance", "http://b.org/prop/nom", "http://b.org/prop/population", "http://b.org/prop/birthDate",
              "http://b.org/prop/areaCodes", "http://b.org/prop/heightCm", "http://b.org/prop/name", "http://b.org/prop/mottos",
              "http://b.org/prop/birthdate", "http://b.org/prop/elevationM", "http://b.org/prop/abbreviations", "http://b.org/prop/founding",
              "http://b.org/prop/lengthKm", "http://b.org/prop/weights", "http://b.org/prop/isbn13", "http://b.org/prop/names"]
    ids1 = {u: i for i, u in enumerate(names1)}
    ids2 = {u: 40 + i for i, u in enumerate(names2)}
    tri1 = [(e, a, "v") for a in ids1.values() for e in range(3 + 2 * a)]
    tri2 = [(e, a, "v") for a in ids2.values() for e in range(1 + 26 * (a - 40))]      # 2 a1 <= 24 < 26: no two pairs share a count
    return ids1, ids2, tri1, tri2


def main():
    import_reference()
    import tf_shim as tf
    lev = types.ModuleType("Levenshtein")
    lev.ratio = ratio
    sys.modules["Levenshtein"] = lev
    ref = importlib.import_module("openea.approaches.imuse")
    from openea_amd.run.default_args import get_args
    rng = random.Random(20190719)
    out = {}

    # ---- the entity step ----------------------------------------------------------------------------------------------------------
    attr_pairs, tri1, tri2 = entity_case(rng)
    threshold = 0.6
    d1, v1 = ref.filter_by_aligned_attributes(tri1, set(a for a, _ in attr_pairs))
    d2, v2 = ref.filter_by_aligned_attributes(tri2, set(a for _, a in attr_pairs))
    one = ref.run_one_ea(d1, d2, v1, v2, threshold, attr_pairs)
    kgs = types.SimpleNamespace(kg1=types.SimpleNamespace(attribute_triples_set=tri1), kg2=types.SimpleNamespace(attribute_triples_set=tri2))
    pool = quiet(ref.align_entity_by_attributes, kgs, attr_pairs, threshold)
    out["entity"] = dict(attr_pairs=attr_pairs, triples1=tri1, triples2=tri2, threshold=threshold,
                         filter1_entities=list(d1.keys()), filter1_attrs=[sorted(s) for s in d1.values()],
                         filter1_values=[[e, a, v] for (e, a), v in v1.items()],
                         filter2_entities=list(d2.keys()), filter2_values=[[e, a, v] for (e, a), v in v2.items()],
                         run_one_ea=sorted(one), align_entity_by_attributes=sorted(pool))
    per_e1 = {}
    for e1, _ in one:
        per_e1[e1] = per_e1.get(e1, 0) + 1
    print("entity step: %d x %d entities, run_one_ea %d pairs (%d entities with more than one), eight chunks + dict %d pairs"
          % (len(d1), len(d2), len(one), sum(c > 1 for c in per_e1.values()), len(pool)))
    assert len(pool) > 10 and max(per_e1.values()) > 1 and sorted(pool) != sorted(one)

    # ---- the name step --------------------------------------------------------------------------------------------------------------
    ids1, ids2, ntri1, ntri2 = name_case()
    nkgs = types.SimpleNamespace(
        kg1=types.SimpleNamespace(attributes_id_dict=ids1, attributes_set=set(ids1.values()), attribute_triples_set=ntri1),
        kg2=types.SimpleNamespace(attributes_id_dict=ids2, attributes_set=set(ids2.values()), attribute_triples_set=ntri2))
    assert list(nkgs.kg1.attributes_set) == sorted(ids1.values()) and list(nkgs.kg2.attributes_set) == sorted(ids2.values())
    top10 = ref.get_aligned_attr_pair_by_name_similarity(nkgs, 0.6)
    top3 = ref.get_aligned_attr_pair_by_name_similarity(nkgs, 0.6, top_k=3)
    top99 = ref.get_aligned_attr_pair_by_name_similarity(nkgs, 0.6, top_k=99)
    out["names"] = dict(ids1=ids1, ids2=ids2, triples1=[[e, a] for e, a, _ in ntri1], triples2=[[e, a] for e, a, _ in ntri2],
                        threshold=0.6, top10=sorted(top10), top3=sorted(top3), all=sorted(top99))
    print("name step: %d pairs found, top 10 %s" % (len(top99), sorted(top10)))
    assert len(top99) > 10 and len(top10) == 10
    # the reference breaks a tie in the triple counts by the iteration order of a set of tuples: keep the counts apart
    counts = [sum(a == a1 for _, a, _ in ntri1) + sum(a == a2 for _, a, _ in ntri2) for a1, a2 in top99]
    assert len(set(counts)) == len(counts), sorted(counts)
    with open(os.path.join(HERE, "imuse.json"), "w", encoding="utf8") as f:
        json.dump(out, f, ensure_ascii=True, indent=0)

    # ---- align_loss and one SGD step ---------------------------------------------------------------------------------------------------
    del tf.VARIABLES[:]
    n_ent, n_rel, d = 14, 4, 5
    m = ref.IMUSE()
    quiet(m.set_args, get_args("IMUSE", dim=d, output="/tmp/oea_golden/", training_data="synthetic/tiny/", dataset_division="f/"))
    m.kgs = types.SimpleNamespace(entities_num=n_ent, relations_num=n_rel)
    m._define_variables()
    m._define_embed_graph()
    variables = list(tf.VARIABLES)
    assert [v.data.shape for v in variables] == [(n_ent, d), (n_rel, d)]
    nrng = np.random.RandomState(7)
    for v in variables:
        v.data = (nrng.standard_normal(v.data.shape) * 0.6).astype(np.float32).astype(np.float64)
    pairs = np.array([[0, 7], [1, 8], [2, 8], [3, 3], [4, 10], [0, 11]], np.int64)     # 8 twice on the right, 0 twice on the left, 3 with itself
    feed = {m.aligned_ents1: pairs[:, 0], m.aligned_ents2: pairs[:, 1]}
    loss = float(tf.evaluate(m.align_loss, feed))
    grads = fd_gradients(tf, m.align_loss, feed, variables)
    assert not grads[1].any()
    lr = float(m.args.learning_rate)
    np.savez_compressed(os.path.join(HERE, "imuse_graph.npz"), align_pairs=pairs, align_loss=np.array([loss]), align_lr=np.array([lr]),
                        align_var_ent_embeds=variables[0].data, align_grad_ent_embeds=grads[0],
                        align_after_ent_embeds=variables[0].data - lr * grads[0])
    print("align_loss %.6f over %d pairs" % (loss, len(pairs)))


if __name__ == "__main__":
    main()
