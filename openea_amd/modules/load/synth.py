"""Seeded synthetic KG pairs with the shapes of the OpenEA benchmark datasets.

The datasets are not vendored (figshare download, reference README.md:187-189) and there is
no network, so every measurement uses these.  Entities get Zipf-like
degrees; every entity occurs in at least one triple; entity i of KG1 is aligned with entity i
of KG2; links are split 20% / 10% / 70% (README.md:252-255).
"""
import os
import random

import numpy as np

from .kg import KG
from .kgs import KGs

# name -> (entities per KG, (#rel1, #rel2), (#triples1, #triples2)); docs/Dataset_Statistics.png
SHAPES = {
    "EN-FR-15K-V1": (15000, (267, 210), (47334, 40864)),
    "D-W-15K-V2": (15000, (167, 121), (73983, 83365)),
    "EN-FR-100K-V1": (100000, (400, 300), (309607, 258285)),
    "EN-DE-100K-V1": (100000, (381, 196), (335359, 336240)),
    "EN-FR-100K-V2": (100000, (379, 287), (649902, 561391)),
    "tiny": (400, (12, 9), (1500, 1300)),
    "small": (3000, (40, 31), (10000, 9000)),
}


# name -> ((#att1, #att2), (#attribute triples1, #attribute triples2)); SURVEY Appendix B for the two benchmark shapes
ATTRIBUTES = {
    "EN-FR-15K-V1": ((308, 404), (73121, 67167)),
    "EN-FR-100K-V1": ((466, 519), (497729, 426672)),
    "tiny": ((24, 30), (1600, 1500)),
    "small": ((40, 48), (14000, 13000)),
}
N_PROFILES = 32


def _zipf_choice(rng, n, size, a=0.9):
    """indices in [0,n) with P(i) ~ (i+1)^-a (hubs at low indices)."""
    w = 1.0 / np.power(np.arange(1, n + 1, dtype=np.float64), a)
    cdf = np.cumsum(w)
    cdf /= cdf[-1]
    return np.minimum(np.searchsorted(cdf, rng.rand(size)), n - 1).astype(np.int64)


def _triples(rng, prefix, n_ent, n_rel, n_tri):
    tri = set()
    # every entity occurs once as a head
    for h, r, t in zip(np.arange(n_ent), _zipf_choice(rng, n_rel, n_ent, 1.1), rng.permutation(n_ent)):
        tri.add((int(h), int(r), int(t)))
    while len(tri) < n_tri:
        m = int((n_tri - len(tri)) * 1.2) + 16
        hs = _zipf_choice(rng, n_ent, m)
        ts = rng.randint(0, n_ent, m)
        rs = _zipf_choice(rng, n_rel, m, 1.1)
        for h, r, t in zip(hs, rs, ts):
            if h != t:
                tri.add((int(h), int(r), int(t)))
                if len(tri) >= n_tri:
                    break
    return {("%s/e%d" % (prefix, h), "%s/r%d" % (prefix, r), "%s/e%d" % (prefix, t)) for h, r, t in tri}


def generate_uri_dataset(shape="EN-FR-15K-V1", seed=0):
    n_ent, (r1, r2), (t1, t2) = SHAPES[shape]
    rng = np.random.RandomState(seed)
    tri1 = _triples(rng, "kg1", n_ent, r1, t1)
    tri2 = _triples(rng, "kg2", n_ent, r2, t2)
    order = rng.permutation(n_ent)
    links = [("kg1/e%d" % i, "kg2/e%d" % i) for i in order]
    n_train, n_valid = int(0.2 * n_ent), int(0.1 * n_ent)
    return tri1, tri2, links[:n_train], links[n_train:n_train + n_valid], links[n_train + n_valid:]


# the alphabet of the synthetic string values: mostly ASCII, a share of accented Latin, Greek and CJK, a few above U+FFFF
_VALUE_ALPHABET = ("abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789 -.,'" * 2
                   + "\u00e9\u00e8\u00e0\u00fc\u00f6\u00e4\u00f1\u00e7\u00df\u00f8\u03b1\u03b2\u03b3\u03b4\u4e2d\u6587\u5b57\u6f22"
                   + "\U0001f600\U00010348\U0001d11e\U00020000")


def _string_value(seed, side, profile, ent, att):
    """The value of (entity ent, attribute att) on KG side `side` as a string of 3 to 40 code points (a few empty, a few above 64
    and above 256): a base string that depends on (profile, ent, att) only, so that the aligned entities of the two KGs share it
    under the attribute of the same number, with 0 to 5 random edits that depend on the side as well."""
    # random.Random seeded with an int (init_by_array of the Mersenne twister) and read through random() alone: the same
    # strings on every Python 3; a numpy RandomState per value costs a millisecond, this a few microseconds
    key = (((int(seed) & 0x7fffffff) * 64 + int(profile)) * (1 << 24) + int(ent)) * (1 << 12) + int(att)
    base = random.Random(key * 4 + 1)
    kind = int(base.random() * 400)
    if kind < 6:
        return ""
    n = 3 + int(base.random() * 38)
    if kind < 10:
        n = 65 + int(base.random() * 65)
    elif kind < 12:
        n = 257 + int(base.random() * 143)
    chars = [_VALUE_ALPHABET[int(base.random() * len(_VALUE_ALPHABET))] for _ in range(n)]
    edit = random.Random(key * 4 + 1 + int(side))
    for _ in range(int(edit.random() * 6)):
        at, what = int(edit.random() * (len(chars) + 1)), int(edit.random() * 3)
        c = _VALUE_ALPHABET[int(edit.random() * len(_VALUE_ALPHABET))]
        if what == 0 or not chars:
            chars.insert(at, c)
        elif what == 1:
            chars[min(at, len(chars) - 1)] = c
        else:
            del chars[min(at, len(chars) - 1)]
    return "".join(chars)


def _attribute_triples(rng, prefix, profile, n_att, n_tri, string_values=None):
    """n_tri (entity, attribute, value) triples over n_att attributes: entity i holds n_tri / n_ent distinct attributes (rounded so
    that the total is exact) drawn without replacement under the weights of its latent profile -- a Zipf law over a
    profile-specific order of the KG's attributes, so that two entities of one profile share most of theirs.
    string_values = (seed, side): the values are _string_value's strings instead of "v<number>"."""
    n_ent = len(profile)
    counts = np.full(n_ent, n_tri // n_ent, np.int64)
    counts[rng.permutation(n_ent)[:n_tri - counts.sum()]] += 1
    counts = np.minimum(counts, n_att)
    logw = -1.5 * np.log(np.arange(1, n_att + 1, dtype=np.float64))
    order = np.stack([rng.permutation(n_att) for _ in range(N_PROFILES)])           # rank of attribute a under profile p
    out = set()
    for lo in range(0, n_ent, 8192):
        hi = min(lo + 8192, n_ent)
        score = logw[order[profile[lo:hi]]] + rng.gumbel(size=(hi - lo, n_att))     # Gumbel top-k = weighted sampling without replacement
        pick = np.argsort(-score, axis=1)
        for i in range(lo, hi):
            for a in pick[i - lo, :counts[i]]:
                value = "v%d" % ((i * 31 + int(a)) % 97) if string_values is None else _string_value(*string_values, profile[i], i, a)
                out.add(("%s/e%d" % (prefix, i), "%s/a%d" % (prefix, a), value))
    return out


def generate_attribute_triples(shape="EN-FR-15K-V1", seed=0, string_values=False):
    """-> (attribute triples of KG1, of KG2) as URI triples.  Entity i of KG1 and entity i of KG2 (aligned) share one latent profile;
    each KG maps a profile to its own attributes, so attribute co-occurrence across the training links carries the signal JAPE's
    Attr2Vec reads.  A stream of its own: the relation triples and links of generate_uri_dataset do not change.
    string_values: the values are strings that IMUSE's similarity can read (_string_value; streams of their own again, so the
    entities' attributes are the same either way); off, the values are "v<number>" as before."""
    n_ent = SHAPES[shape][0]
    (a1, a2), (t1, t2) = ATTRIBUTES[shape]
    rng = np.random.RandomState([seed, 0xa77])
    profile = rng.randint(0, N_PROFILES, n_ent)
    return (_attribute_triples(rng, "kg1", profile, a1, t1, (seed, 1) if string_values else None),
            _attribute_triples(rng, "kg2", profile, a2, t2, (seed, 2) if string_values else None))


def literal_vectors(literals, dim, seed=0, literal_len=5):
    """A stand-in for MultiKE's literal encoder (the reference encodes word vectors of a 1 M-word file with an auto-encoder):
    the mean of per-word vectors, standard normal and seeded by (seed, crc32(word)), over the first literal_len words of a
    literal; a literal without a word takes the empty word's vector -> float32 [len(literals), dim]."""
    import zlib
    cache = {}

    def word(w):
        if w not in cache:
            cache[w] = np.random.RandomState([int(seed) & 0x7fffffff, zlib.crc32(w.encode('utf-8'))]).standard_normal(dim)
        return cache[w]
    out = np.zeros((len(literals), dim), np.float32)
    for i, literal in enumerate(literals):
        words = literal.split()[:literal_len] or ['']
        out[i] = np.mean([word(w) for w in words], axis=0)
    return out


def make_kgs(shape="EN-FR-15K-V1", mode="mapping", ordered=True, seed=0, verbose=False, attributes=False, string_values=False):
    """-> KGs built through the same id-assignment code as a real dataset.  attributes=True adds generate_attribute_triples (for
    the shapes in ATTRIBUTES); the default has none, as before.  string_values=True (with attributes): string values."""
    tri1, tri2, train, valid, test = generate_uri_dataset(shape, seed)
    att1, att2 = generate_attribute_triples(shape, seed, string_values) if attributes else (set(), set())
    return KGs(KG(tri1, att1, verbose=verbose), KG(tri2, att2, verbose=verbose), train, test, valid_links=valid,
               mode=mode, ordered=ordered, verbose=verbose)


def write_dataset(folder, shape="tiny", seed=0, division="721_5fold/1/"):
    """write the reference's folder layout (README.md:204-220) for end-to-end runs."""
    tri1, tri2, train, valid, test = generate_uri_dataset(shape, seed)
    os.makedirs(os.path.join(folder, division), exist_ok=True)

    def dump(path, rows):
        with open(path, "w", encoding="utf8") as f:
            for row in rows:
                f.write("\t".join(row) + "\n")
    dump(os.path.join(folder, "rel_triples_1"), sorted(tri1))
    dump(os.path.join(folder, "rel_triples_2"), sorted(tri2))
    dump(os.path.join(folder, "attr_triples_1"), [])
    dump(os.path.join(folder, "attr_triples_2"), [])
    dump(os.path.join(folder, "ent_links"), train + valid + test)
    dump(os.path.join(folder, division, "train_links"), train)
    dump(os.path.join(folder, division, "valid_links"), valid)
    dump(os.path.join(folder, division, "test_links"), test)
    return folder
