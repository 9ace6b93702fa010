"""GPU parity tests: HIP kernels (through the C ABI) vs the oracle on the same seeded inputs.

Integer outputs (ranks, argmax, neighbour sets, sampled negatives) must be bit-exact;
floating-point tables within the tolerance written next to each assert."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ops():
    from openea_amd import ops as _ops
    _ops.lib()   # raises loudly if the HIP library / GPU is missing
    return _ops


def _embeds(rng, n1, n2, d, noise=0.8):
    e1 = rng.standard_normal((n1, d)).astype(np.float32) / np.sqrt(d)
    e2 = rng.standard_normal((n2, d)).astype(np.float32) / np.sqrt(d)
    e2[:n1] = e1 + noise * rng.standard_normal((n1, d)).astype(np.float32) / np.sqrt(d)
    return e1, e2


# ---------------------------------------------------------------------------------------------
# similarity / rank
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1,n2,d", [(300, 420, 40), (1000, 1500, 100), (129, 129, 75), (1, 1, 8), (257, 700, 300), (260, 900, 1200),
                                     (131, 300, 500)])
@pytest.mark.parametrize("metric", ["inner", "manhattan", "euclidean"])
def test_rank_eval_bit_exact(ops, n1, n2, d, metric):
    from oracle import cport
    rng = np.random.RandomState(n1 + d)
    e1, e2 = _embeds(rng, n1, n2, d)
    rank, argmax = ops.rank_eval(ops.to_table(e1), ops.to_table(e2), d, metric)
    r_ref, a_ref = cport.rank_eval(e1, e2, metric)
    assert np.array_equal(rank.cpu().numpy(), r_ref)
    assert np.array_equal(argmax.cpu().numpy(), a_ref)


@pytest.mark.parametrize("metric", ["inner", "manhattan", "euclidean"])
def test_sim_matrix_bit_exact(ops, metric):
    from oracle import cport
    rng = np.random.RandomState(3)
    e1, e2 = _embeds(rng, 200, 333, 100)
    s = ops.sim_matrix(ops.to_table(e1), ops.to_table(e2), 100, metric).cpu().numpy()
    ref = cport.sim_matrix(e1, e2, metric)
    if metric == "euclidean":   # sqrt rounding: device sqrt vs libm, 1 ulp
        np.testing.assert_allclose(s, ref, rtol=0, atol=2e-7)
    else:
        assert np.array_equal(s, ref)   # MFMA fp32 == k-ordered fmaf chain; fp64 L1 == scipy order


def test_rank_ties_and_duplicates(ops):
    """exact ties: duplicated candidate rows -> stable order (smaller column first)."""
    from oracle import cport
    rng = np.random.RandomState(5)
    e1, e2 = _embeds(rng, 64, 200, 16)
    e2[100:164] = e2[:64]          # every gold has an exact duplicate at a LARGER column
    e2[170:180] = e2[20:30]        # and some a third copy
    e1[7] = 0.0                    # an all-zero query: every similarity ties at 0
    rank, argmax = ops.rank_eval(ops.to_table(e1), ops.to_table(e2), 16, "inner")
    r_ref, a_ref = cport.rank_eval(e1, e2, "inner")
    assert np.array_equal(rank.cpu().numpy(), r_ref)
    assert np.array_equal(argmax.cpu().numpy(), a_ref)
    assert r_ref[7] == 7 and a_ref[7] == 0


def test_csls_pipeline_bit_exact(ops):
    from oracle import cport, np_oracle as orc
    rng = np.random.RandomState(11)
    e1, e2 = _embeds(rng, 250, 400, 64)
    t1, t2 = ops.to_table(e1), ops.to_table(e2)
    s = ops.sim_matrix(t1, t2, 64, "inner")
    st = ops.sim_matrix(t2, t1, 64, "inner")
    r = ops.row_topk_mean(s, 10)
    c = ops.row_topk_mean(st, 10)
    s_ref = cport.sim_matrix(e1, e2, "inner")
    r_ref = cport.topk_mean(s_ref, 10, axis=1)
    c_ref = cport.topk_mean(s_ref, 10, axis=0)
    assert np.array_equal(r.cpu().numpy(), r_ref)
    assert np.array_equal(c.cpu().numpy(), c_ref)
    rank, argmax = ops.rank_eval(t1, t2, 64, "inner", csls_r=r, csls_c=c)
    rk_ref, am_ref = cport.rank_eval(e1, e2, "inner", r_ref, c_ref)
    assert np.array_equal(rank.cpu().numpy(), rk_ref)
    assert np.array_equal(argmax.cpu().numpy(), am_ref)
    # materialised CSLS matrix == oracle csls_sim
    ops.csls_apply_(s, r, c)
    assert np.array_equal(s.cpu().numpy(), orc.csls_sim(s_ref, 10))


def test_rank_metrics(ops):
    from oracle import np_oracle as orc
    rng = np.random.RandomState(2)
    rank = rng.randint(0, 3000, 12345).astype(np.int32)
    hits, rs, rr = ops.rank_metrics(ops.to_ids(rank), [1, 5, 10, 50])
    h_ref, _, mr, mrr = orc.metrics_from_ranks(rank, [1, 5, 10, 50], len(rank))
    assert hits == h_ref
    assert rs == int((rank.astype(np.int64) + 1).sum())
    assert abs(rr / len(rank) - mrr) < 1e-12


@pytest.mark.parametrize("n1,n2,d,csls", [(300, 420, 40, False), (1000, 1500, 100, True), (129, 129, 75, False), (1, 1, 8, False),
                                          (10500, 10500, 75, False), (2500, 7000, 100, True)])
def test_rank_eval_metrics_two_launches_equal_the_separate_calls(ops, n1, n2, d, csls):
    """oea_rank_eval_metrics (prologue + sweep whose last workgroup extracts argmax and reduces the metrics) == oea_rank_eval
    + oea_rank_metrics == the oracle, bit for bit -- also called twice in a row (the ticket counter is reset by the prologue)."""
    from oracle import cport
    rng = np.random.RandomState(n1 + d)
    e1, e2 = _embeds(rng, n1, n2, d)
    t1, t2 = ops.to_table(e1), ops.to_table(e2)
    r = c = None
    if csls:
        s = ops.sim_matrix(t1, t2, d, "inner")
        r, c = ops.row_topk_mean(s, 10), ops.row_topk_mean(ops.sim_matrix(t2, t1, d, "inner"), 10)
    top_k = [1, 5, 10, 50]
    rank0, am0 = ops.rank_eval(t1, t2, d, "inner", csls_r=r, csls_c=c)
    hits0, rs0, rr0 = ops.rank_metrics(rank0, top_k)
    for _ in range(2):
        rank, am, hits, rs, rr = ops.rank_eval_metrics(t1, t2, d, top_k, r, c)
        assert np.array_equal(rank.cpu().numpy(), rank0.cpu().numpy()) and np.array_equal(am.cpu().numpy(), am0.cpu().numpy())
        assert hits == hits0 and rs == rs0 and abs(rr - rr0) <= 1e-9 * max(rr0, 1.0)
    if n1 <= 1000:
        r_ref, a_ref = cport.rank_eval(e1, e2, "inner", None if r is None else r.cpu().numpy(), None if c is None else c.cpu().numpy())
        assert np.array_equal(rank.cpu().numpy(), r_ref) and np.array_equal(am.cpu().numpy(), a_ref)


@pytest.mark.parametrize("n2,k", [(1031, 10), (12, 10), (64, 1), (5000, 32), (257, 16)])
def test_row_topk_mean_edge_cases(ops, n2, k):
    """calculate_nearest_k (similarity.py:80-83): ties, constant rows (more than 256 entries at the threshold ->
    insertion fallback), -inf entries, short rows, rows that are not 16-byte aligned; bit-exact vs the oracle."""
    import torch
    from oracle import cport
    rng = np.random.RandomState(n2 + k)
    rows = [rng.standard_normal(n2), np.zeros(n2), np.round(rng.standard_normal(n2) * 3) / 3,
            np.where(rng.rand(n2) < 0.5, -np.inf, rng.standard_normal(n2)), -np.arange(n2, dtype=np.float64),
            np.arange(n2, dtype=np.float64)]
    s = np.stack(rows).astype(np.float32)
    if np.isinf(s[3]).sum() > n2 - k:
        s[3, :k] = 1.0
    ref = cport.topk_mean(s, k, axis=1)
    got = ops.row_topk_mean(torch.from_numpy(s).to(ops.device()), k).cpu().numpy()
    assert np.array_equal(got, ref)


def test_calculate_rank_block_matches_oracle(ops):
    """calculate_rank (alignment.py:146-168) on an explicit row block with ties: oea_rank_rows."""
    from oracle import np_oracle as orc
    from openea_amd.modules.finding.alignment import calculate_rank
    rng = np.random.RandomState(7)
    sim_mat = np.round(rng.standard_normal((97, 1031)) * 4).astype(np.float32) / 4      # heavy ties
    sim_mat[::2] *= np.float32(-0.0) + 1
    idx = rng.randint(0, 1031, 97)
    got = calculate_rank(idx, sim_mat, [1, 5, 10], True, 97)
    ref = orc.calculate_rank(idx, sim_mat, [1, 5, 10], True, 97)
    assert got[0] == ref[0] and abs(got[1] - ref[1]) < 1e-12
    assert list(got[2]) == list(ref[2]) and got[3] == ref[3]


@pytest.mark.parametrize("csls_k", [0, 5])
def test_stable_alignment_matches_oracle(ops, csls_k, capsys):
    """stable_alignment (alignment.py:87-134): device similarity + top-`cut` candidate lists + the reference's
    Gale-Shapley loop == the oracle's full-argsort version on the same similarity matrix."""
    from oracle import np_oracle as orc
    from openea_amd.modules.finding.alignment import stable_alignment
    from openea_amd.modules.finding.similarity import sim
    rng = np.random.RandomState(3)
    e1 = rng.standard_normal((180, 24)).astype(np.float32)
    e2 = (e1 + 0.8 * rng.standard_normal((180, 24))).astype(np.float32)
    for cut in (100, 7):
        got = stable_alignment(e1, e2, "inner", True, csls_k, 1, cut=cut)
        ref = orc.stable_alignment(sim(e1, e2, metric="inner", normalize=True, csls_k=csls_k), cut)
        assert got == ref
    assert "stable alignment precision = " in capsys.readouterr().out


# ---------------------------------------------------------------------------------------------
# neighbour search
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,k", [(600, 32, 59), (2000, 100, 199), (1500, 75, 1), (300, 16, 300)])
def test_topk_inner_bit_exact(ops, n, d, k):
    from oracle import cport
    rng = np.random.RandomState(n)
    emb = rng.standard_normal((n, d)).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    emb[5] = emb[9]                       # duplicated rows -> boundary ties exist for some queries
    t = ops.to_table(emb)
    idx = ops.topk_inner(t, t, d, k).cpu().numpy()
    ref = cport.topk_inner(emb, emb, k)
    assert np.array_equal(idx, ref)
    # chunked workspace path gives the same answer
    idx2 = ops.topk_inner(t, t, d, k, ws_bytes=128 * ((n + 31) // 32 * 32) * 4).cpu().numpy()
    assert np.array_equal(idx2, ref)


def _select_ref(s, k):
    """(value desc, column asc) selection, ascending columns -- the rule of oracle_topk_inner."""
    out = np.empty((s.shape[0], k), np.int32)
    for i, row in enumerate(s):
        order = np.lexsort((np.arange(len(row)), -row.astype(np.float64)))
        out[i] = np.sort(order[:k])
    return out


@pytest.mark.parametrize("nc,k", [(5000, 500), (1027, 37), (257, 257), (3, 2)])
def test_topk_rows_ties_and_ragged(ops, nc, k):
    import torch
    rng = np.random.RandomState(nc)
    ld = (nc + 31) // 32 * 32
    rows = []
    rows.append(np.zeros(nc, np.float32))                                   # constant row: radix path, first k columns
    rows.append(rng.randint(0, 4, nc).astype(np.float32))                   # 4 distinct values: radix path
    rows.append(np.round(rng.standard_normal(nc) * 40).astype(np.float32))  # quantised: ties inside the buckets
    x = rng.standard_normal(nc).astype(np.float32); x[rng.randint(0, nc, max(nc // 8, 1))] = 1e30
    rows.append(x)                                                          # outliers: clamped end buckets
    x = rng.standard_normal(nc).astype(np.float32); x[::2] = -0.0; x[1::4] = 0.0
    rows.append(x)                                                          # signed zeros compare equal
    rows.append(np.sort(rng.standard_normal(nc).astype(np.float32)))        # sampled range misses nothing / ascending
    rows.append(-np.sort(rng.standard_normal(nc).astype(np.float32)))
    s = np.stack(rows)
    sp_ = np.full((len(rows), ld), np.nan, np.float32)                      # pad columns must never be selected
    sp_[:, :nc] = s
    got = ops.topk_rows(torch.from_numpy(sp_).to(ops.device()), k, nc=nc).cpu().numpy()
    assert np.array_equal(got, _select_ref(s, k))


@pytest.mark.parametrize("nc,k", [(20000, 1500), (16384, 64), (33333, 3000), (12000, 1100), (2052, 700)])
def test_topk_rows_sampled_path(ops, nc, k):
    """rows long enough for the one-read (sampled threshold) select, including rows built to defeat the sample, and rows of
    2,048 .. 32,768 columns that the select holds in LDS (one read of the strip; tie-heavy rows take its radix path on the
    LDS copy): whatever path a row takes, the (value desc, column asc) selection is the oracle's."""
    import torch
    rng = np.random.RandomState(nc + k)
    ld = (nc + 31) // 32 * 32
    runs = np.zeros(nc, bool)                                    # the columns the kernel samples
    for b in range(64):
        st = (b * (nc - 128) // 63) & ~3
        runs[st:st + 128] = True
    rows = [rng.standard_normal(nc), np.zeros(nc), np.round(rng.standard_normal(nc) * 2) / 2]
    x = rng.standard_normal(nc); x[runs] += 10.0                 # sample far above the rest: too few candidates -> 3-pass
    rows.append(x)
    x = rng.standard_normal(nc); x[~runs] += 10.0                # sample far below the rest: every entry a candidate -> overflow
    rows.append(x)
    x = rng.standard_normal(nc) * 1e-3; x[rng.choice(nc, k // 2, replace=False)] = 5.0
    rows.append(x)                                               # half of the top-k are outliers
    rows.append(np.sort(rng.standard_normal(nc)))
    rows.append(rng.standard_normal(nc) ** 3)                    # heavy tails
    s = np.stack(rows).astype(np.float32)
    sp_ = np.full((len(rows), ld), np.nan, np.float32)
    sp_[:, :nc] = s
    got = ops.topk_rows(torch.from_numpy(sp_).to(ops.device()), k, nc=nc).cpu().numpy()
    assert np.array_equal(got, _select_ref(s, k))
    ids = rng.permutation(nc).astype(np.int32)
    got = ops.topk_rows(torch.from_numpy(sp_).to(ops.device()), k, id_map=ops.to_ids(ids), nc=nc).cpu().numpy()
    assert np.array_equal(got, ids[_select_ref(s, k)])


def test_topk_matches_reference_fixture(ops, golden_dir):
    g = np.load(os.path.join(golden_dir, "neighbours.npz"))
    emb, ents, k = g['emb'], g['entity_list'], int(g['k'])
    t = ops.to_table(emb)
    out = ops.topk_inner(t, t, emb.shape[1], k, id_map=ops.to_ids(ents)).cpu().numpy()
    assert np.array_equal(out, g['nbrs'])     # the reference's own neighbour sets (sorted)


# ---------------------------------------------------------------------------------------------
# negative sampler
# ---------------------------------------------------------------------------------------------
def test_sampler_bit_exact_vs_oracle(ops, golden_dir):
    from oracle import cport
    g = np.load(os.path.join(golden_dir, "neg_sampling.npz"))
    triples, ents, pos, nbr = g['triples'], g['entity_list'], g['pos'], g['nbr']
    ent_pos = np.full(int(ents.max()) + 1, -1, np.int32)
    ent_pos[ents] = np.arange(len(ents), dtype=np.int32)
    table_ref = cport.tripleset_build(triples)
    d_tri = ops.to_ids(triples)
    table = ops.tripleset_build(d_tri)
    torch.cuda.synchronize()
    # same membership (slot order may differ because inserts race; the key SET must agree)
    assert sorted(table.cpu().numpy().view(np.uint64).tolist()) == sorted(table_ref.tolist())
    for use_nbr in (False, True):
        for step in (0, 3):
            out, err = ops.sample_negatives(ops.to_ids(pos), 10, table, ops.to_ids(ents),
                                            ent_pos=ops.to_ids(ent_pos) if use_nbr else None,
                                            nbr=ops.to_ids(nbr) if use_nbr else None, seed=0xC0FFEE1234, step=step,
                                            pos_offset=17)
            ref = cport.sample_negatives(pos, 10, table_ref, ents, ent_pos if use_nbr else None,
                                         nbr if use_nbr else None, seed=0xC0FFEE1234, step=step, pos_offset=17)
            assert int(err.item()) == 0
            assert np.array_equal(out.cpu().numpy(), ref)


def test_sampler_membership_filter_changes_nothing(ops):
    """oea_tripleset_filter_build (round 6): the "certainly absent" bit array in front of the membership probes (batch.py:108-110) has
    no false negatives -- every present triple's bit is set -- and the sampler's output with it equals the output without it, on a
    DENSE graph (40 % of all (h, r, t) are triples: most draws of the first rounds are rejected) and on a sparse one; both equal the
    oracle."""
    from oracle import cport
    rng = np.random.RandomState(4)
    for n_ent, n_rel, dens in ((60, 3, 0.4), (3000, 20, 2e-5)):
        ents = np.arange(n_ent, dtype=np.int32)
        allt = np.stack(np.meshgrid(ents, np.arange(n_rel, dtype=np.int32), ents, indexing="ij"), -1).reshape(-1, 3) if n_ent < 100 else \
            np.unique(np.stack([rng.randint(0, n_ent, 4000), rng.randint(0, n_rel, 4000), rng.randint(0, n_ent, 4000)], 1), axis=0).astype(np.int32)
        triples = allt[rng.rand(len(allt)) < dens] if n_ent < 100 else allt
        triples = np.ascontiguousarray(triples, np.int32)
        pos = triples[rng.choice(len(triples), min(len(triples), 1500), replace=False)]
        d_tri, d_ents = ops.to_ids(triples), ops.to_ids(ents)
        table = ops.tripleset_build(d_tri)
        filt = ops.tripleset_filter(d_tri, table.numel())
        bits = filt.cpu().numpy().view(np.uint32)
        nb = 32 * len(bits)
        assert nb == 8 * table.numel()
        assert 0 < int(np.unpackbits(bits.view(np.uint8)).sum()) <= len(triples)            # at most one bit per triple
        ent_pos = ops.to_ids(np.arange(n_ent, dtype=np.int32))
        outs = []
        for f in (None, filt):
            side = ops.sampler_side(table, d_ents, ent_pos, None, f)
            out = torch.empty((len(pos) * 10, 3), dtype=torch.int32, device=d_tri.device)
            err = torch.zeros(1, dtype=torch.int32, device=d_tri.device)
            ops.sample_negatives_pair(ops.to_ids(pos), len(pos), 10, side, side, 77, 5, 0, out, err)
            assert int(err.item()) == 0
            outs.append(out.cpu().numpy())
        assert np.array_equal(outs[0], outs[1])
        ref = cport.sample_negatives(pos, 10, cport.tripleset_build(triples), ents, None, None, seed=77, step=5, pos_offset=0)
        assert np.array_equal(outs[1], ref)
        # no false negatives: a filter built over the triples answers "maybe present" for each of them -- sampling the positives'
        # own (h, r, t) as candidates would be rejected; checked through the bits directly with the kernel's hash restated here
        def mix64(x):                                            # csrc/common.h: splitmix64's finaliser
            x = np.uint64(x)
            with np.errstate(over="ignore"):
                x ^= x >> np.uint64(30); x *= np.uint64(0xBF58476D1CE4E5B9)
                x ^= x >> np.uint64(27); x *= np.uint64(0x94D049BB133111EB)
                x ^= x >> np.uint64(31)
            return x
        keys = (triples[:, 0].astype(np.uint64) << np.uint64(40)) | (triples[:, 1].astype(np.uint64) << np.uint64(24)) | triples[:, 2].astype(np.uint64)
        b = np.array([int(mix64(k ^ np.uint64(0x9E3779B97F4A7C15))) & (nb - 1) for k in keys[:500]], np.int64)
        assert ((bits[b >> 5] >> (b & 31).astype(np.uint32)) & 1).all()


def test_sampler_neighbour_fallback_and_k64(ops):
    """entities without a neighbour row (ent_pos = -1: the other KG's entities inside seed-swapped
    triples) fall back to the whole entity list; k > 16 uses the 64-lane groups."""
    from oracle import cport
    rng = np.random.RandomState(9)
    n_ent = 300
    ents = np.arange(0, 2 * n_ent, 2).astype(np.int32)             # this KG: even ids
    triples = np.unique(np.stack([rng.choice(ents, 2000), rng.randint(0, 7, 2000), rng.choice(ents, 2000)], 1), axis=0).astype(np.int32)
    pos = triples[:200].copy()
    pos[::3, 0] = 2 * rng.randint(0, n_ent, len(pos[::3])) + 1     # odd ids: no neighbour row
    ent_pos = np.full(2 * n_ent, -1, np.int32)
    ent_pos[ents] = np.arange(n_ent, dtype=np.int32)
    nbr = np.stack([rng.choice(ents, 70, replace=False) for _ in range(n_ent)]).astype(np.int32)
    table_ref = cport.tripleset_build(triples)
    table = ops.tripleset_build(ops.to_ids(triples))
    for k in (10, 40, 64):
        out, err = ops.sample_negatives(ops.to_ids(pos), k, table, ops.to_ids(ents), ent_pos=ops.to_ids(ent_pos),
                                        nbr=ops.to_ids(nbr), seed=77, step=5)
        ref = cport.sample_negatives(pos, k, table_ref, ents, ent_pos, nbr, seed=77, step=5)
        assert int(err.item()) == 0
        assert np.array_equal(out.cpu().numpy(), ref)
        got = out.cpu().numpy().reshape(len(pos), k, 3)
        assert np.all(got[:, :, 1] == pos[:, None, 1])             # relation preserved
        assert np.all((got[:, :, 0] == pos[:, None, 0]) | (got[:, :, 2] == pos[:, None, 2]))


@pytest.mark.parametrize("case", ["truncated", "uniform", "dense"])
def test_device_sampler_replays_the_reference_run(ops, golden_dir, case):
    """sample_negatives_kernel fed the RECORDED draws of a run of the reference's generate_neg_triples_fast
    (oea_sample_negatives_replay; tests/golden/neg_replay.npz) instead of Philox: the reference's negatives, every positive's
    family as a multiset, and the oracle's replay slot for slot -- the sampler's algorithm (rounds, one side per round, removal of
    true triples except in the last round) pinned against the reference itself, not only against its restatement."""
    from oracle import np_oracle
    g = np.load(os.path.join(golden_dir, "neg_replay.npz"))
    nbr = None
    if case == "dense":
        tri, ents, pos, k, max_try = g["dense_triples"], g["dense_entities"], g["dense_pos"], 5, 3
        ch = ct = [ents] * len(pos)
    else:
        s = np.load(os.path.join(golden_dir, "neg_sampling.npz"))
        tri, ents, pos, k, max_try = s["triples"], s["entity_list"], s["pos"], 10, 10
        row = {int(e): i for i, e in enumerate(ents)}
        if case == "truncated":
            nbr = s["nbr"]
        ch = [s["nbr"][row[int(h)]] if case == "truncated" else ents for h in pos[:, 0]]
        ct = [s["nbr"][row[int(t)]] if case == "truncated" else ents for t in pos[:, 2]]
    replay, ref = g["replay_" + case], g["neg_" + case]
    ent_pos = np.full(int(ents.max()) + 1, -1, np.int32)
    ent_pos[ents] = np.arange(len(ents), dtype=np.int32)
    table = ops.tripleset_build(ops.to_ids(tri))
    out, err = ops.sample_negatives_replay(ops.to_ids(pos), k, table, ops.to_ids(ents), torch.from_numpy(replay).to(ops.device()),
                                           ent_pos=ops.to_ids(ent_pos) if nbr is not None else None,
                                           nbr=ops.to_ids(nbr) if nbr is not None else None, max_try=max_try)
    assert int(err.item()) == 0
    got = out.cpu().numpy()
    fam = lambda a: [sorted(map(tuple, f.tolist())) for f in np.asarray(a).reshape(-1, k, 3)]      # noqa: E731
    assert fam(got) == fam(ref)
    assert np.array_equal(got, np_oracle.sample_negatives_replay(pos, k, tri, ch, ct, replay, max_try))


# ---------------------------------------------------------------------------------------------
# translational step
# ---------------------------------------------------------------------------------------------
def _kg(rng, n_ent, n_rel, n_pos, k):
    pos = np.stack([rng.randint(0, n_ent, n_pos), rng.randint(0, n_rel, n_pos), rng.randint(0, n_ent, n_pos)], 1).astype(np.int32)
    neg = np.repeat(pos, k, axis=0)
    flip = rng.rand(len(neg)) < 0.5
    neg[flip, 0] = rng.randint(0, n_ent, int(flip.sum()))
    neg[~flip, 2] = rng.randint(0, n_ent, int((~flip).sum()))
    return pos, neg


STEP_CASES = [
    dict(loss="limited", loss_norm="L2", pos_margin=0.01, neg_margin=2.0, balance=0.2, k=10, d=100),   # BootEA / AlignE
    dict(loss="limited", loss_norm="L2", pos_margin=0.01, neg_margin=2.0, balance=0.2, k=10, d=75),    # BASELINE dim=75
    dict(loss="margin-based", loss_norm="L1", margin=1.5, k=1, d=64),
    dict(loss="margin-based", loss_norm="L2", margin=1.0, k=1, d=300, rel_l2_norm=False),
    dict(loss="logistic", loss_norm="L2", k=3, d=32, ent_l2_norm=False, rel_l2_norm=False, optimizer="SGD", lr=0.05),
    dict(loss="positive", loss_norm="L2", k=0, d=100),                                                # MTransE
    dict(loss="align", loss_norm="L2", k=0, d=100),                                                   # BootEA alignment loss
    dict(loss="limited", loss_norm="L1", pos_margin=0.5, neg_margin=4.0, balance=1.0, k=2, d=1200),
]


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("case", STEP_CASES, ids=lambda c: "%s-%s-d%d" % (c["loss"], c["loss_norm"], c["d"]))
def test_triple_step_vs_oracle(ops, case, grouped):
    from oracle import cport
    case = dict(case)
    k, d = case.pop("k"), case.pop("d")
    if grouped and (k == 0 or case["loss"] == "margin-based"):
        pytest.skip("grouped layout applies to per-triple losses with negatives")
    rng = np.random.RandomState(d + k)
    n_ent, n_rel, n_pos = 700, 23, 900
    ent = (rng.standard_normal((n_ent, d)) / np.sqrt(d)).astype(np.float32) * 1.3
    rel = (rng.standard_normal((n_rel, d)) / np.sqrt(d)).astype(np.float32) * 0.7
    ent_acc = np.full_like(ent, 0.1)
    rel_acc = np.full_like(rel, 0.1)
    pos, neg = _kg(rng, n_ent, n_rel, n_pos, max(k, 1))
    if k == 0:
        neg = None
    cfg_kw = dict(loss=case.get("loss"), loss_norm=case.get("loss_norm"), margin=case.get("margin", 0.0),
                  pos_margin=case.get("pos_margin", 0.0), neg_margin=case.get("neg_margin", 0.0),
                  balance=case.get("balance", 1.0), ent_l2_norm=case.get("ent_l2_norm", True),
                  rel_l2_norm=case.get("rel_l2_norm", True), optimizer=case.get("optimizer", "Adagrad"),
                  lr=case.get("lr", 0.01))
    ld = ops.pad4(d)
    d_ent, d_rel = ops.to_table(ent), ops.to_table(rel)
    d_eacc, d_racc = ops.to_table(ent_acc), ops.to_table(rel_acc)
    d_eacc[:, d:] = 0.1
    d_racc[:, d:] = 0.1
    ws = ops.step_workspace(n_ent, n_rel, ld)
    loss_acc = torch.zeros(1, dtype=torch.float64, device=d_ent.device)
    if grouped and neg is not None:
        # a few entries that are NOT corruptions of their positive: must still be scored correctly
        neg[5] = (3, 2, 9)
        neg[40] = neg[41]
    cfg = ops.make_step_cfg(neg_group_k=k if grouped else 0, **cfg_kw)
    d_pos = ops.to_ids(pos)
    d_neg = ops.to_ids(neg) if neg is not None else None
    losses_ref = []
    for it in range(3):      # three consecutive steps: exercises workspace re-zeroing + accumulators
        ops.triple_step(d_ent, d_eacc, d_rel, d_racc, d, d_pos, d_neg, cfg, ws, loss_acc)
        losses_ref.append(cport.triple_step(ent, ent_acc, rel, rel_acc, pos, neg, **cfg_kw))
    torch.cuda.synchronize()
    got_ent = d_ent.cpu().numpy()
    got_rel = d_rel.cpu().numpy()
    # embedding L2 within 1e-4 (north_star tolerance) PER ROW, measured deviation printed (pytest -s)
    from _tol import assert_rows_close
    assert_rows_close(got_ent[:, :d], ent, "entity table after 3 steps")
    assert_rows_close(got_rel[:, :d], rel, "relation table after 3 steps")
    assert np.all(got_ent[:, d:] == 0) and np.all(got_rel[:, d:] == 0)      # pad columns stay zero
    assert abs(loss_acc.item() - sum(losses_ref)) <= 1e-4 * abs(sum(losses_ref)) + 1e-6
    # gradient scratch + touched flags are left clean (the tail holds the loss partials)
    assert not bool((ws[: ws.numel() - 8 * 4096] != 0).any().item())
    if cfg_kw["optimizer"] == "Adagrad":
        np.testing.assert_allclose(d_eacc.cpu().numpy()[:, :d], ent_acc, rtol=2e-4, atol=1e-7)


@pytest.mark.parametrize("d,k,l1", [(100, 10, False), (128, 3, False), (128, 10, False), (100, 3, False), (75, 7, True), (200, 10, False),
                                    (64, 1, False), (37, 10, True), (256, 5, False)])
def test_triple_step_one_sided_negatives_vs_oracle(ops, d, k, l1):
    """The sampler's layout -- all k negatives of a positive corrupt the SAME side (one Bernoulli per round, batch.py:101-107) --
    is what triple_wave's select-free loops take (the mixed-side batches of test_triple_step_vs_oracle go through its
    independent-triple path): three Adagrad steps of the limited loss against the C oracle, per-row 1e-4, at every fragment
    count (ld <= 64 / 128 / 256), k = 10 (compile-time) and k < 10 (run-time), both norms; a self-loop, a negative equal to its
    positive and an entity that is head of forty positives ride along."""
    from oracle import cport
    from _tol import assert_rows_close
    rng = np.random.RandomState(1000 * d + k)
    n_ent, n_rel, n_pos = 900, 19, 1100
    ent = (rng.standard_normal((n_ent, d)) / np.sqrt(d)).astype(np.float32) * 1.3
    rel = (rng.standard_normal((n_rel, d)) / np.sqrt(d)).astype(np.float32) * 0.7
    ent_acc, rel_acc = np.full_like(ent, 0.1), np.full_like(rel, 0.1)
    pos = np.stack([rng.randint(0, n_ent, n_pos), rng.randint(0, n_rel, n_pos), rng.randint(0, n_ent, n_pos)], 1).astype(np.int32)
    pos[11, 2] = pos[11, 0]
    pos[100:140, 0] = 7
    neg = np.repeat(pos, k, axis=0)
    flip = np.repeat(rng.rand(n_pos) < 0.5, k)
    neg[flip, 0] = rng.randint(0, n_ent, int(flip.sum()))
    neg[~flip, 2] = rng.randint(0, n_ent, int((~flip).sum()))
    neg[3 * k] = pos[3]
    kw = dict(loss="limited", loss_norm="L1" if l1 else "L2", pos_margin=0.01 if not l1 else 0.5, neg_margin=2.0 if not l1 else 4.0,
              balance=0.2, optimizer="Adagrad", lr=0.01)
    ld = ops.pad4(d)
    d_ent, d_rel = ops.to_table(ent), ops.to_table(rel)
    d_eacc, d_racc = ops.to_table(ent_acc), ops.to_table(rel_acc)
    d_eacc[:, d:] = 0.1
    d_racc[:, d:] = 0.1
    ws = ops.step_workspace(n_ent, n_rel, ld)
    loss_acc = torch.zeros(1, dtype=torch.float64, device=d_ent.device)
    cfg = ops.make_step_cfg(neg_group_k=k, **kw)
    d_pos, d_neg = ops.to_ids(pos), ops.to_ids(neg)
    loss_ref = 0.0
    for _ in range(3):
        ops.triple_step(d_ent, d_eacc, d_rel, d_racc, d, d_pos, d_neg, cfg, ws, loss_acc)
        loss_ref += cport.triple_step(ent, ent_acc, rel, rel_acc, pos, neg, **kw)
    torch.cuda.synchronize()
    assert_rows_close(d_ent.cpu().numpy()[:, :d], ent, "entity table after 3 steps")
    assert_rows_close(d_rel.cpu().numpy()[:, :d], rel, "relation table after 3 steps")
    assert abs(loss_acc.item() - loss_ref) <= 1e-4 * abs(loss_ref) + 1e-6
    assert not bool((ws[: ws.numel() - 8 * 4096] != 0).any().item())          # scratch + flags left clean


def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("d", [75, 100, 300, 37, 500, 1200])
def test_bf16_prefilter_evaluation_equals_the_fp32_sweep(ops, d, monkeypatch):
    """oea_rank_eval[_metrics]_bf16: the tile sweep multiplies bf16 splits (hi.hi + hi.lo + lo.hi on v_mfma_f32_32x32x16_bf16),
    counts what the error bound decides and records the rest for the exact k-ordered chain.  (1) the approximate similarities
    stay inside the certified bound; (2) ranks, nearest candidates and the integer metrics equal the fp32 sweep's on random
    golds (hundreds of records), golds near the top, exact duplicates of gold columns in front of and behind them (the tie rule),
    unnormalised rows, and a clustered table whose records overflow (the caller's fallback to the fp32 sweep)."""
    rng = np.random.RandomState(d)
    a, b = _unit(rng.standard_normal((700, d))), _unit(rng.standard_normal((1300, d)))
    ta, tb = ops.to_table(a), ops.to_table(b)
    err = float((ops.sim_matrix(ta, tb, d, "inner") - ops.sim_bf16_matrix(ta, tb, d)).abs().max())
    # the certificate (csrc/sim_rank.hip:bf16_eps_rel, K blocks of 128): split residue + the products of ONE block (+ one rounding
    # per block sum) at a chopping 2^-23 + the exact chain's own roundings at 2^-24 -- 1.3e-4 instead of 5.9e-4 at d = 1,200
    kp16 = (d + 15) // 16 * 16
    blocks = (kp16 + 127) // 128
    n_acc = 3 * 128 + blocks if blocks > 1 else 3 * kp16
    assert err <= 1.02 * (3.02 * 2.0 ** -18 + n_acc * 2.0 ** -23 + (d + 8) * 2.0 ** -24), err
    n1, n2, off = 1500, 4000, 700
    e2 = _unit(rng.standard_normal((n2, d)))
    e2t = e2.copy()
    e2t[3000:3400] = e2t[off:off + 400]
    e2t[0:300] = e2t[off + 500:off + 800]
    e2c = e2.copy()
    e2c[1000:3000] = _unit(e2c[1000] + 2e-4 * rng.standard_normal((2000, d)))
    e2u = (e2 * rng.uniform(0.05, 4.0, (n2, 1))).astype(np.float32)
    cases = {"random gold": (_unit(rng.standard_normal((n1, d))), e2),
             "gold near the top": (_unit(e2[off:off + n1] + 0.5 * rng.standard_normal((n1, d)) / np.sqrt(d)), e2),
             "duplicated gold columns": (_unit(e2t[off:off + n1] + 0.1 * rng.standard_normal((n1, d)) / np.sqrt(d)), e2t),
             "unnormalised rows": ((e2u[off:off + n1] + 0.3 * rng.standard_normal((n1, d)).astype(np.float32) / np.sqrt(d)).astype(np.float32), e2u),
             "clustered (overflow)": (_unit(e2c[off:off + n1] + 1e-4 * rng.standard_normal((n1, d))), e2c)}
    monkeypatch.setenv("OEA_EVAL_BF16", "0")
    for name, (q, c) in cases.items():
        t1, t2 = ops.to_table(q), ops.to_table(c)
        r0, a0 = ops.rank_eval(t1, t2, d, "inner", gold_offset=off)
        st = {}
        r1, a1 = ops.rank_eval_bf16(t1, t2, d, gold_offset=off, stats=st)
        assert torch.equal(r0, r1) and torch.equal(a0, a1), (name, st)
        assert st["fallback"] == name.startswith("clustered"), (name, st)
        if not name.startswith("clustered"):       # a block of query rows with its gold offset AND CSLS terms (the sharded evaluation)
            g = torch.Generator(device=t1.device).manual_seed(3)
            rr = torch.rand(t1.shape[0], device=t1.device, generator=g) * 0.3
            cc = torch.rand(t2.shape[0], device=t1.device, generator=g) * 0.3
            r0c, a0c = ops.rank_eval(t1, t2, d, "inner", rr, cc, gold_offset=off)
            r1c, a1c = ops.rank_eval_bf16(t1, t2, d, gold_offset=off, csls_r=rr, csls_c=cc)
            assert torch.equal(r0c, r1c) and torch.equal(a0c, a1c), name
        if off == 0 or True:
            q0, c0 = ops.to_table(q), ops.to_table(c[off:])         # the metrics entry point takes gold_offset too; use 0 here
            m0 = ops.rank_eval_metrics(q0, c0, d, [1, 5, 10, 50])
            m1 = ops.rank_eval_metrics_bf16(q0, c0, d, [1, 5, 10, 50])
            if name.startswith("clustered"):
                assert m1 is None
            else:
                assert torch.equal(m0[0], m1[0]) and torch.equal(m0[1], m1[1]) and m0[2] == m1[2] and m0[3] == m1[3], name
                assert abs(m0[4] - m1[4]) <= 1e-9 * abs(m0[4])
                # the same with CSLS means: (2 s - r) - c ranked from the approximate s + exact records
                from openea_amd.modules.finding.similarity import csls_means_device
                rr, cc = csls_means_device(q0, c0, d, "inner", 10)
                m0 = ops.rank_eval_metrics(q0, c0, d, [1, 5, 10, 50], rr, cc)
                m1 = ops.rank_eval_metrics_bf16(q0, c0, d, [1, 5, 10, 50], csls_r=rr, csls_c=cc)
                assert m1 is not None and torch.equal(m0[0], m1[0]) and torch.equal(m0[1], m1[1]) and m0[2] == m1[2] and m0[3] == m1[3], name


def test_greedy_alignment_takes_the_bf16_prefilter_and_reports_the_same(ops, monkeypatch):
    """greedy_alignment_device routes inner-product evaluations of >= OEA_EVAL_BF16_MIN_PAIRS pairs (3e8 by default) through
    oea_rank_eval_metrics_bf16, with and without CSLS means; everything it returns equals the fp32 sweep's."""
    from openea_amd.modules.finding.alignment import greedy_alignment_device
    rng = np.random.RandomState(5)
    n, d = 2600, 75
    e2 = _unit(rng.standard_normal((n, d)))
    e1 = _unit(e2 + 0.6 * rng.standard_normal((n, d)) / np.sqrt(d))
    t1, t2 = ops.to_table(e1), ops.to_table(e2)
    assert not ops.eval_bf16_enabled(10500, 10500) and ops.eval_bf16_enabled(70000, 70000)
    for csls in (0, 10):
        monkeypatch.setenv("OEA_EVAL_BF16", "0")
        r0, a0, h0, rs0, rr0 = greedy_alignment_device(t1, t2, d, [1, 5, 10, 50], "inner", False, csls)
        monkeypatch.setenv("OEA_EVAL_BF16", "1")
        monkeypatch.setenv("OEA_EVAL_BF16_MIN_PAIRS", "1")
        assert ops.eval_bf16_enabled(n, n)
        calls = []
        real = ops.rank_eval_metrics_bf16
        monkeypatch.setattr(ops, "rank_eval_metrics_bf16", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
        r1, a1, h1, rs1, rr1 = greedy_alignment_device(t1, t2, d, [1, 5, 10, 50], "inner", False, csls)
        monkeypatch.setattr(ops, "rank_eval_metrics_bf16", real)
        monkeypatch.delenv("OEA_EVAL_BF16_MIN_PAIRS")
        assert calls and torch.equal(r0, r1) and torch.equal(a0, a1) and list(h0) == list(h1) and rs0 == rs1
        assert abs(rr0 - rr1) <= 1e-9 * abs(rr0)


DET_WORKER = r'''
import os, sys
import numpy as np
import torch
sys.path.insert(0, os.environ["OEA_ROOT"]); sys.path.insert(0, os.path.join(os.environ["OEA_ROOT"], "tests"))
from openea_amd import ops
from oracle import cport
assert ops.deterministic() == (os.environ["OEA_STEP_DETERMINISTIC"] == "1")
rng = np.random.RandomState(110)
n_ent, n_rel, n_pos, k, d = 700, 23, 900, 10, 100
ent0 = (rng.standard_normal((n_ent, d)) / np.sqrt(d)).astype(np.float32) * 1.3
rel0 = (rng.standard_normal((n_rel, d)) / np.sqrt(d)).astype(np.float32) * 0.7
pos = np.stack([rng.randint(0, n_ent, n_pos), rng.randint(0, n_rel, n_pos), rng.randint(0, n_ent, n_pos)], 1).astype(np.int32)
neg = np.repeat(pos, k, 0)
flip = rng.rand(len(neg)) < 0.5
neg[flip, 0] = rng.randint(0, n_ent, int(flip.sum()))
neg[~flip, 2] = rng.randint(0, n_ent, int((~flip).sum()))
kw = dict(loss="limited", loss_norm="L2", pos_margin=0.01, neg_margin=2.0, balance=0.2, optimizer="Adagrad", lr=0.01)
runs = []
for run in range(2):
    e, r = ops.to_table(ent0), ops.to_table(rel0)
    ea, ra = torch.full_like(e, 0.1), torch.full_like(r, 0.1)
    ws = ops.step_workspace(n_ent, n_rel, ops.pad4(d))
    loss = torch.zeros(1, dtype=torch.float64, device=e.device)
    cfg = ops.make_step_cfg(neg_group_k=k, **kw)
    for _ in range(3):
        ops.triple_step(e, ea, r, ra, d, ops.to_ids(pos), ops.to_ids(neg), cfg, ws, loss)
    torch.cuda.synchronize()
    runs.append((e.cpu().numpy()[:, :d], r.cpu().numpy()[:, :d], float(loss.item())))
ent, rel = ent0.copy(), rel0.copy()
ea, ra = np.full_like(ent, 0.1), np.full_like(rel, 0.1)
for _ in range(3):
    cport.triple_step(ent, ea, rel, ra, pos, neg, **kw)
dev = lambda a, b: float((np.linalg.norm(a.astype(np.float64) - b, axis=1) / np.maximum(np.linalg.norm(b, axis=1), 1.0)).max())
print("RESULT same_bits=%d ent_dev=%.3e rel_dev=%.3e" % (int(np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
                                                             and runs[0][2] == runs[1][2]), dev(runs[0][0], ent), dev(runs[0][1], rel)))
'''


def test_fixed_point_build_is_reproducible_and_closer_to_the_oracle(capsys):
    """libopenea_hip_det.so (OEA_STEP_DETERMINISTIC=1): the gradient sums are int64 fixed point -- two runs of three BootEA-style
    steps (900 positives x 11, hubs and relation rows with hundreds of contributions) give the SAME BITS, and the tables sit
    within 2e-6 per row of the oracle (fp64 internals: the exact row sums are what it computes); the fp32-atomics build is
    held to the north-star 1e-4 and need not repeat its bits."""
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = {}
    for det in ("0", "1"):
        p = subprocess.run([sys.executable, "-c", DET_WORKER], env=dict(os.environ, OEA_ROOT=root, OEA_STEP_DETERMINISTIC=det),
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        m = re.search(r"RESULT same_bits=(\d) ent_dev=(\S+) rel_dev=(\S+)", p.stdout)
        out[det] = (int(m.group(1)), float(m.group(2)), float(m.group(3)))
    with capsys.disabled():
        print("\nthree steps vs the oracle, max row deviation (entity / relation): fp32 atomics %.2e / %.2e (same bits twice: %d), "
              "fixed point %.2e / %.2e (same bits twice: %d)" % (out["0"][1], out["0"][2], out["0"][0], out["1"][1], out["1"][2], out["1"][0]))
    assert out["1"][0] == 1 and out["1"][1] <= 2e-6 and out["1"][2] <= 2e-6
    assert out["0"][1] <= 1e-4 and out["0"][2] <= 1e-4


# ---------------------------------------------------------------------------------------------
# graph aggregate + GCN-Align epoch
# ---------------------------------------------------------------------------------------------
def _random_graph(rng, n, avg_deg):
    import scipy.sparse as sp
    nnz = n * avg_deg
    rows = np.minimum((rng.zipf(1.7, nnz) - 1), n - 1)
    cols = rng.randint(0, n, nnz)
    vals = rng.rand(nnz).astype(np.float32)
    a = sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()
    a.sum_duplicates()
    a.sort_indices()
    return a


@pytest.mark.parametrize("d", [100, 64, 300, 500])
def test_spmm_bit_exact(ops, d):
    from oracle import cport
    rng = np.random.RandomState(d)
    n = 1200
    a = _random_graph(rng, n, 8)
    x = rng.standard_normal((n, d)).astype(np.float32)
    coo = a.tocoo()      # row-sorted, same within-row order as the CSR
    ref = cport.spmm_coo(coo.row, coo.col, coo.data, x, n)
    y = ops.spmm_csr(ops.to_ids(a.indptr), ops.to_ids(a.indices), ops.to_vec(a.data),
                     ops.to_table(x), d)
    short = np.diff(a.indptr) <= 96          # rows summed serially in CSR order: bit-exact
    assert (~short).sum() > 0                # the Zipf graph has hub rows: workgroup-cooperative path
    got = y.cpu().numpy()[:, :d]
    assert np.array_equal(got[short], ref[short])
    np.testing.assert_allclose(got[~short], ref[~short], rtol=2e-5, atol=5e-4)   # ~1000-term fp32 sums in another order
    yr = ops.spmm_csr(ops.to_ids(a.indptr), ops.to_ids(a.indices), ops.to_vec(a.data),
                      ops.to_table(x), d, act=1)
    np.testing.assert_allclose(yr.cpu().numpy()[:, :d], np.maximum(ref, 0), rtol=2e-5, atol=5e-4)
    # hub rows cut into chunks over several workgroups (oea_csr_split), with relu + mask epilogue
    split = ops.csr_split(a.indptr, threshold=200, chunk=128)
    assert split is not None and split.n_chunks > split.n_rows
    mask = rng.standard_normal((n, d)).astype(np.float32)
    ym = ops.spmm_csr(ops.to_ids(a.indptr), ops.to_ids(a.indices), ops.to_vec(a.data), ops.to_table(x), d,
                      act=1, mask_from=ops.to_table(mask), split=split)
    np.testing.assert_allclose(ym.cpu().numpy()[:, :d], np.maximum(ref, 0) * (mask > 0), rtol=2e-5, atol=5e-4)
    assert np.array_equal(ym.cpu().numpy()[short][:, :d], (np.maximum(ref, 0) * (mask > 0))[short])


# ---------------------------------------------------------------------------------------------
# TransH scoring (approaches/bootea_transh.py:58-96)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,k,loss,opt", [(40, 5, "limited", "Adagrad"), (75, 10, "limited", "Adagrad"),
                                           (100, 3, "logistic", "SGD"), (32, 0, "positive", "Adagrad")])
def test_transh_step_matches_oracle(ops, d, k, loss, opt):
    import torch
    from oracle import cport
    rng = np.random.RandomState(d + k)
    n_ent, n_rel, n_pos = 600, 17, 400
    ent = rng.standard_normal((n_ent, d)).astype(np.float32)
    rel = rng.standard_normal((n_rel, d)).astype(np.float32)
    nrm = rng.standard_normal((n_rel, d)).astype(np.float32)
    pos = np.stack([rng.randint(0, n_ent, n_pos), np.minimum(rng.zipf(1.6, n_pos) - 1, n_rel - 1),
                    rng.randint(0, n_ent, n_pos)], 1).astype(np.int32)
    neg = None
    if k:
        neg = np.repeat(pos, k, axis=0)
        ch = rng.rand(n_pos * k) < 0.5
        rnd = rng.randint(0, n_ent, n_pos * k)
        neg[ch, 0] = rnd[ch]
        neg[~ch, 2] = rnd[~ch]
        neg[7] = [3, 2, 5]                                 # entries that are not corruptions of their positive
        neg[8, 1] = (neg[8, 1] + 1) % n_rel
    kw = dict(loss=loss, loss_norm="L2", pos_margin=0.01, neg_margin=2.0, balance=0.2, optimizer=opt, lr=0.01)
    # oracle
    e0, r0, n0 = ent.copy(), rel.copy(), nrm.copy()
    ea, ra, na = (np.full_like(x, 0.1) for x in (e0, r0, n0))
    ref_loss = 0.0
    for _ in range(2):                                     # two steps: accumulators + a clean scratch in between
        ref_loss += cport.triple_step_transh(e0, ea, r0, ra, n0, na, pos, neg, **kw)
    # device
    te, tr, tn = ops.to_table(ent), ops.to_table(rel), ops.to_table(nrm)
    tea, tra, tna = (torch.full_like(x, 0.1) for x in (te, tr, tn))
    cfg = ops.make_step_cfg(neg_group_k=k, normal=tn, normal_acc=tna, **kw)
    ws = ops.step_workspace(n_ent, n_rel, te.shape[1])
    acc = torch.zeros(1, dtype=torch.float64, device=te.device)
    for _ in range(2):
        ops.triple_step(te, tea, tr, tra, d, ops.to_ids(pos), None if neg is None else ops.to_ids(neg), cfg, ws, acc)
    assert abs(float(acc.item()) - ref_loss) <= 2e-5 * abs(ref_loss)
    for got, ref in ((te, e0), (tr, r0), (tn, n0)):
        assert np.linalg.norm(got[:, :d].cpu().numpy() - ref) <= 1e-4 * np.linalg.norm(ref)
    assert int(ws[: -8 * 4096].count_nonzero()) == 0       # scratch (incl. the normal-vector copies) left clean
    # the exchange-split step (data parallelism) gives the same update
    te2, tr2, tn2 = ops.to_table(ent), ops.to_table(rel), ops.to_table(nrm)
    tea2, tra2, tna2 = (torch.full_like(x, 0.1) for x in (te2, tr2, tn2))
    cfg2 = ops.make_step_cfg(neg_group_k=k, normal=tn2, normal_acc=tna2, **kw)
    for _ in range(2):
        for phase in (ops.PHASE_GRAD, ops.PHASE_APPLY):
            ops.triple_step(te2, tea2, tr2, tra2, d, ops.to_ids(pos), None if neg is None else ops.to_ids(neg), cfg2, ws, acc, phase=phase)
    for a, b in ((te, te2), (tr, tr2), (tn, tn2)):
        assert np.linalg.norm((a - b).cpu().numpy()) <= 2e-6 * np.linalg.norm(a.cpu().numpy())


@pytest.mark.parametrize("d,loss,free_list", [(40, "margin-based", False), (100, "margin-based", False),
                                              (75, "limited", True), (300, "margin-based", False)])
def test_transh_margin_and_free_lists_match_oracle(ops, d, loss, free_list):
    """models/trans/transh.py:16-51: margin pairs (pos i, neg i) -- and a per-triple loss on an UNGROUPED negative
    list (3 negatives for 400 positives: not the sampler layout) -- take the one-item-per-group kernel."""
    import torch
    from oracle import cport
    rng = np.random.RandomState(d)
    n_ent, n_rel, n_pos = 500, 13, 400
    ent, rel, nrm = (rng.standard_normal((n, d)).astype(np.float32) for n in (n_ent, n_rel, n_rel))
    pos = np.stack([rng.randint(0, n_ent, n_pos), np.minimum(rng.zipf(1.6, n_pos) - 1, n_rel - 1),
                    rng.randint(0, n_ent, n_pos)], 1).astype(np.int32)
    n_neg = 3 if free_list else n_pos
    neg = np.stack([rng.randint(0, n_ent, n_neg), rng.randint(0, n_rel, n_neg), rng.randint(0, n_ent, n_neg)], 1).astype(np.int32)
    kw = dict(loss=loss, loss_norm="L2", margin=1.5, pos_margin=0.01, neg_margin=2.0, balance=0.2, optimizer="Adagrad", lr=0.01)
    e0, r0, n0 = ent.copy(), rel.copy(), nrm.copy()
    ea, ra, na = (np.full_like(x, 0.1) for x in (e0, r0, n0))
    ref_loss = sum(cport.triple_step_transh(e0, ea, r0, ra, n0, na, pos, neg, **kw) for _ in range(2))
    te, tr, tn = ops.to_table(ent), ops.to_table(rel), ops.to_table(nrm)
    tea, tra, tna = (torch.full_like(x, 0.1) for x in (te, tr, tn))
    cfg = ops.make_step_cfg(neg_group_k=0, normal=tn, normal_acc=tna, **kw)
    ws = ops.step_workspace(n_ent, n_rel, te.shape[1])
    acc = torch.zeros(1, dtype=torch.float64, device=te.device)
    for _ in range(2):
        ops.triple_step(te, tea, tr, tra, d, ops.to_ids(pos), ops.to_ids(neg), cfg, ws, acc)
    assert ref_loss > 0 and abs(float(acc.item()) - ref_loss) <= 2e-5 * abs(ref_loss)
    for got, ref in ((te, e0), (tr, r0), (tn, n0)):
        assert np.linalg.norm(got[:, :d].cpu().numpy() - ref) <= 1e-4 * np.linalg.norm(ref)
    assert int(ws[: -8 * 4096].count_nonzero()) == 0


@pytest.mark.parametrize("d,loss,l1,opt", [(40, "margin-based", False, "Adagrad"), (100, "margin-based", False, "Adagrad"),
                                           (75, "margin-based", True, "SGD"), (64, "limited", False, "Adagrad"),
                                           (200, "margin-based", False, "Adagrad")])
def test_transd_step_matches_oracle(ops, d, loss, l1, opt):
    """OEA_SCORE_TRANSD (models/trans/transd.py:16-57) on stacked tables against oracle_triple_step_transd, two steps,
    plus the exchange-split form."""
    import torch
    from oracle import cport
    rng = np.random.RandomState(d + 1)
    E, R, n_pos = 450, 11, 380
    ent = rng.standard_normal((2 * E, d)).astype(np.float32)
    rel = rng.standard_normal((2 * R, d)).astype(np.float32)
    pos = np.stack([rng.randint(0, E, n_pos), np.minimum(rng.zipf(1.6, n_pos) - 1, R - 1), rng.randint(0, E, n_pos)], 1).astype(np.int32)
    neg = pos.copy()
    ch = rng.rand(n_pos) < 0.5
    rnd = rng.randint(0, E, n_pos)
    neg[ch, 0] = rnd[ch]
    neg[~ch, 2] = rnd[~ch]
    kw = dict(loss=loss, loss_norm="L1" if l1 else "L2", margin=1.0, pos_margin=0.01, neg_margin=2.5, balance=0.3,
              optimizer=opt, lr=0.01)
    e0, r0 = ent.copy(), rel.copy()
    ea, ra = np.full_like(e0, 0.1), np.full_like(r0, 0.1)
    ref_loss = sum(cport.triple_step_transd(e0, ea, r0, ra, pos, neg, **kw) for _ in range(2))
    assert ref_loss > 0

    def device_run(split):
        te, tr = ops.to_table(ent), ops.to_table(rel)
        tea, tra = torch.full_like(te, 0.1), torch.full_like(tr, 0.1)
        cfg = ops.make_step_cfg(neg_group_k=0, transfer_bases=(E, R), **kw)
        ws = ops.step_workspace(2 * E, 2 * R, te.shape[1])
        acc = torch.zeros(1, dtype=torch.float64, device=te.device)
        for _ in range(2):
            for phase in ((ops.PHASE_GRAD, ops.PHASE_APPLY) if split else (ops.PHASE_BOTH,)):
                ops.triple_step(te, tea, tr, tra, d, ops.to_ids(pos), ops.to_ids(neg), cfg, ws, acc, phase=phase)
        assert int(ws[: -8 * 4096].count_nonzero()) == 0
        return te, tr, float(acc.item())

    te, tr, loss_dev = device_run(False)
    assert abs(loss_dev - ref_loss) <= 2e-5 * abs(ref_loss)
    for got, ref in ((te, e0), (tr, r0)):
        assert np.linalg.norm(got[:, :d].cpu().numpy() - ref) <= 1e-4 * np.linalg.norm(ref)
    assert np.abs(te[E:, :d].cpu().numpy() - ent[E:]).max() > 1e-4       # the transfer vectors were trained
    te2, tr2, _ = device_run(True)
    for a, b in ((te, te2), (tr, tr2)):
        assert np.linalg.norm((a - b).cpu().numpy()) <= 2e-6 * np.linalg.norm(a.cpu().numpy())
    # ids outside [0, base) / tables that are not stacked are refused
    with pytest.raises(RuntimeError):
        bad = ops.make_step_cfg(neg_group_k=0, transfer_bases=(E - 1, R), **kw)
        ops.triple_step(te, torch.full_like(te, 0.1), tr, torch.full_like(tr, 0.1), d, ops.to_ids(pos), ops.to_ids(neg), bad,
                        ops.step_workspace(2 * E, 2 * R, te.shape[1]), torch.zeros(1, dtype=torch.float64, device=te.device))


# ---------------------------------------------------------------------------------------------
# RotatE step in fp64 (approaches/bootea_rotate.py:50-109,148-158)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,k,opt,ent_norm,rel_norm", [(100, 10, "Adam", True, False), (40, 3, "Adagrad", True, True),
                                                       (75, 0, "Adam", True, False), (200, 2, "SGD", False, False),
                                                       (300, 1, "Adam", True, False), (32, 17, "Adam", True, False)])
def test_rotate_step_matches_oracle(ops, d, k, opt, ent_norm, rel_norm):
    """three steps (Adam's bias correction and moments, a clean scratch) against np_oracle.rotate_step; k = 0 is the
    alignment loss (positives only); one negative is not a corruption of its positive; k = 17 spreads a family over two
    lane groups (chunks of 16); d = 300 runs without the register accumulation of the family rows; the split step agrees."""
    import torch
    from oracle import np_oracle as orc
    rng = np.random.RandomState(d + k)
    E, R, n_pos = 400, 9, 350
    ent = rng.standard_normal((2 * E, d)) / np.sqrt(d)
    rel = rng.standard_normal((R, d)) / np.sqrt(d)
    pos = np.stack([rng.randint(0, E, n_pos), np.minimum(rng.zipf(1.6, n_pos) - 1, R - 1), rng.randint(0, E, n_pos)], 1).astype(np.int32)
    neg = None
    if k:
        neg = np.repeat(pos, k, axis=0)
        ch = rng.rand(n_pos * k) < 0.5
        rnd = rng.randint(0, E, n_pos * k)
        neg[ch, 0] = rnd[ch]
        neg[~ch, 2] = rnd[~ch]
        neg[5, 1] = (neg[5, 1] + 1) % R
    cfg = ops.make_rotate_cfg(6.0, d, ent_l2_norm=ent_norm, rel_l2_norm=rel_norm, optimizer=opt, lr=0.01)
    kw = dict(gamma=6.0, phase_scale=cfg.phase_scale, ent_l2_norm=ent_norm, rel_l2_norm=rel_norm, optimizer=opt, lr=0.01)
    assert abs(cfg.phase_scale - np.pi / (8.0 / d)) < 1e-9
    e0, r0, st = ent.copy(), rel.copy(), {}
    ref_loss = sum(orc.rotate_step(e0, r0, pos, neg, st, **kw) for _ in range(3))

    def device_run(split):
        te, tr = ops.to_table64(ent), ops.to_table64(rel)
        se, sr = ops.rotate_state(te, opt), ops.rotate_state(tr, opt)
        ws = ops.rotate_workspace(E, R, te.shape[1])
        acc = torch.zeros(1, dtype=torch.float64, device=te.device)
        dpos, dneg = ops.to_ids(pos), None if neg is None else ops.to_ids(neg)
        for step in range(3):
            cfg.t = step + 1
            for phase in ((ops.PHASE_GRAD, ops.PHASE_APPLY) if split else (ops.PHASE_BOTH,)):
                ops.rotate_step(te, se, tr, sr, d, dpos, dneg, k, cfg, ws, acc, phase=phase)
        assert int(ws[: -8 * 4096].count_nonzero()) == 0
        return te, tr, float(acc.item())

    te, tr, loss_dev = device_run(False)
    assert abs(loss_dev - ref_loss) <= 1e-10 * abs(ref_loss)
    for got, ref in ((te, e0), (tr, r0)):
        assert np.linalg.norm(got[:, :d].cpu().numpy() - ref) <= 1e-9 * np.linalg.norm(ref)
        assert float(got[:, d:].abs().sum()) == 0.0
    te2, tr2, _ = device_run(True)
    for a, b in ((te, te2), (tr, tr2)):
        # two runs differ by the order of their fp64 atomics only; the unnormalised phase rows amplify that rounding
        # noise by phase_scale (observed up to 4e-12 relative over three steps at d = 200)
        assert np.linalg.norm((a - b).cpu().numpy()) <= 1e-10 * np.linalg.norm(a.cpu().numpy())
    # the lookups evaluation reads
    ids = rng.permutation(E)[:97].astype(np.int32)
    for part_norm, sum_norm in ((True, False), (True, True), (False, True)):
        got = ops.rotate_lookup(te, d, ops.to_ids(ids), part_norm, sum_norm)
        ref = orc.rotate_lookup(te[:, :d].cpu().numpy(), ids, part_norm, sum_norm)
        assert got.shape[1] % 4 == 0 and float(got[:, d:].abs().sum()) == 0.0
        np.testing.assert_allclose(got[:, :d].cpu().numpy(), ref, rtol=0, atol=1e-7)


# ---------------------------------------------------------------------------------------------
# negative links (AliNet.generate_input_batch, alinet.py:988-1006)
# ---------------------------------------------------------------------------------------------
def test_link_negatives_bit_exact_and_set_semantics(ops):
    import torch
    from oracle import np_oracle as orc
    rng = np.random.RandomState(5)
    n_ent = 900
    ents1 = rng.permutation(n_ent)[:400].astype(np.int32)
    ents2 = (n_ent + rng.permutation(n_ent)[:380]).astype(np.int32)
    sup = [(int(ents1[i]), int(ents2[i])) for i in range(0, 120)]
    excl = ops.tripleset_build(ops.to_ids(np.asarray([(a, 0, b) for a, b in sup], np.int32)))
    # uniform
    n_pos, k = 150, 4
    pairs, valid, scratch = ops.sample_link_negatives(n_pos, k, ents1=ops.to_ids(ents1), ents2=ops.to_ids(ents2), exclude=excl,
                                                      seed=77, step=3)
    ref_p, ref_v = orc.link_negatives(n_pos, k, 77, 3, ents1=ents1, ents2=ents2, exclude=sup)
    assert np.array_equal(pairs.cpu().numpy(), ref_p) and np.array_equal(valid.cpu().numpy() > 0, ref_v)
    p = pairs.cpu().numpy().reshape(k, n_pos, 2)
    for r in range(k):                                     # random.sample: no repeats inside a round, members of the lists
        assert len(set(p[r, :, 0])) == n_pos and len(set(p[r, :, 1])) == n_pos
    assert set(p[..., 0].ravel()) <= set(ents1) and set(p[..., 1].ravel()) <= set(ents2)
    kept = {tuple(x) for x, v in zip(pairs.cpu().numpy().tolist(), valid.cpu().numpy()) if v > 0}
    assert kept == set(map(tuple, ref_p.tolist())) - set(sup) and int((valid > 0).sum()) == len(kept)
    # every entity about equally often over many steps (uniform sampling)
    cnt = np.zeros(2 * n_ent)
    for step in range(40):
        q, _, scratch = ops.sample_link_negatives(n_pos, k, ents1=ops.to_ids(ents1), ents2=ops.to_ids(ents2), seed=1, step=step, scratch=scratch)
        np.add.at(cnt, q.cpu().numpy().ravel(), 1)
    c1 = cnt[ents1]
    assert c1.min() > 0 and abs(c1.mean() - 40 * k * n_pos / len(ents1)) < 1e-9 and c1.std() < 0.2 * c1.mean()
    # truncated
    nbr_k = 37
    nbr1 = np.stack([rng.permutation(ents2)[:nbr_k] for _ in ents1]).astype(np.int32)
    nbr2 = np.stack([rng.permutation(ents1)[:nbr_k] for _ in ents2]).astype(np.int32)
    row1 = np.full(2 * n_ent, -1, np.int32); row1[ents1] = np.arange(len(ents1))
    row2 = np.full(2 * n_ent, -1, np.int32); row2[ents2] = np.arange(len(ents2))
    idx = rng.randint(0, 120, 90)                         # positives drawn WITH replacement (alinet.py:986): duplicate links
    pos = np.asarray([sup[i] for i in idx], np.int32)
    k = 6
    pairs, valid, _ = ops.sample_link_negatives(len(pos), k, pos_links=ops.to_ids(pos), nbr1=ops.to_ids(nbr1), row1=ops.to_ids(row1),
                                                nbr2=ops.to_ids(nbr2), row2=ops.to_ids(row2), exclude=excl, seed=9, step=1)
    ref_p, ref_v = orc.link_negatives(len(pos), k, 9, 1, pos_links=pos, nbr1=nbr1, row1=row1, nbr2=nbr2, row2=row2, exclude=sup)
    assert np.array_equal(pairs.cpu().numpy(), ref_p) and np.array_equal(valid.cpu().numpy() > 0, ref_v)
    assert (~ref_v).sum() > 0                              # duplicates / supervised pairs were really dropped
    pp = pairs.cpu().numpy().reshape(len(pos), 2, k, 2)
    for i, (e1, e2) in enumerate(pos):
        assert len(set(pp[i, 0, :, 1])) == k and set(pp[i, 0, :, 1]) <= set(nbr1[row1[e1]]) and (pp[i, 0, :, 0] == e1).all()
        assert len(set(pp[i, 1, :, 0])) == k and set(pp[i, 1, :, 0]) <= set(nbr2[row2[e2]]) and (pp[i, 1, :, 1] == e2).all()
    with pytest.raises(Exception, match="Sample larger than population"):
        ops.sample_link_negatives(500, 2, ents1=ops.to_ids(ents1), ents2=ops.to_ids(ents2))


def test_step_with_empty_shard_is_a_clean_noop(ops):
    """data parallelism: a rank whose slice of a batch is empty still joins the exchange -- GRAD with no rows, then
    APPLY: tables untouched when nothing was exchanged, and no stale loss partial is added."""
    import torch
    rng = np.random.RandomState(0)
    ent = ops.to_table(rng.standard_normal((50, 16)).astype(np.float32))
    rel = ops.to_table(rng.standard_normal((5, 16)).astype(np.float32))
    ea, ra = torch.full_like(ent, 0.1), torch.full_like(rel, 0.1)
    cfg = ops.make_step_cfg(loss="limited", pos_margin=0.01, neg_margin=2.0, balance=0.2, neg_group_k=2)
    ws = ops.step_workspace(50, 5, ent.shape[1])
    loss = torch.zeros(1, dtype=torch.float64, device=ent.device)
    pos = ops.to_ids(np.array([[1, 2, 3], [4, 0, 5]], np.int32))
    neg = ops.to_ids(np.array([[1, 2, 9], [7, 2, 3], [4, 0, 8], [6, 0, 5]], np.int32))
    ops.triple_step(ent, ea, rel, ra, 16, pos, neg, cfg, ws, loss)            # leaves loss partials behind
    l1, e1 = float(loss.item()), ent.clone()
    empty = torch.zeros((0, 3), dtype=torch.int32, device=ent.device)
    for phase in (ops.PHASE_GRAD, ops.PHASE_APPLY):
        ops.triple_step(ent, ea, rel, ra, 16, empty, None, cfg, ws, loss, phase=phase)
    assert float(loss.item()) == l1 and torch.equal(ent, e1)


# ---------------------------------------------------------------------------------------------
# MTransE mapping step (modules/base/mapping.py:9-19, losses.py:76-80)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n,opt", [(75, 250, "Adagrad"), (32, 37, "SGD"), (130, 64, "Adagrad")])
def test_mapping_step_matches_oracle(ops, d, n, opt):
    import torch
    from oracle import np_oracle as orc
    rng = np.random.RandomState(d)
    n_ent = 900
    ent = rng.standard_normal((n_ent, d)).astype(np.float32)
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    M = (q + 0.05 * rng.standard_normal((d, d))).astype(np.float32)
    links = np.stack([rng.choice(n_ent, n, replace=False), rng.choice(n_ent, n, replace=False)], 1).astype(np.int32)
    links[3, 0] = links[5, 0]                                   # a repeated entity: gradients are summed
    alpha, lr = 5.0, 0.01
    e0, m0 = ent.copy(), M.copy()
    ea0, ma0 = np.full_like(e0, 0.1), np.full_like(m0, 0.1)
    ref_loss = 0.0
    for _ in range(2):
        if opt == "Adagrad":
            ref_loss += orc.mapping_step(e0, m0, ea0, ma0, links, alpha, lr)
        else:                                                   # SGD restated from the same gradients
            v = e0.astype(np.float64); Mm = m0.astype(np.float64)
            inv = 1.0 / np.sqrt(np.maximum((v ** 2).sum(1, keepdims=True), 1e-12)); y = v * inv
            e1, e2 = y[links[:, 0]], y[links[:, 1]]
            diff = e2 - e1 @ Mm; orth = Mm @ Mm.T - np.eye(d)
            ref_loss += alpha * ((diff ** 2).sum() + (orth ** 2).sum())
            gy = np.zeros_like(v); np.add.at(gy, links[:, 0], -2 * alpha * diff @ Mm.T); np.add.at(gy, links[:, 1], 2 * alpha * diff)
            gv = (gy - y * (y * gy).sum(1, keepdims=True)) * inv
            e0 = (v - lr * gv).astype(np.float32)
            m0 = (Mm - lr * alpha * (-2.0 * e1.T @ diff + 4.0 * orth @ Mm)).astype(np.float32)
    te = ops.to_table(ent)
    tm = torch.from_numpy(M).to(te.device).contiguous()
    tea, tma = torch.full_like(te, 0.1), torch.full_like(tm, 0.1)
    rel = ops.to_table(rng.standard_normal((3, d)).astype(np.float32))
    cfg = ops.make_step_cfg(loss="positive", optimizer=opt, lr=lr)
    ws = ops.step_workspace(n_ent, 3, te.shape[1])
    loss = torch.zeros(1, dtype=torch.float64, device=te.device)
    dummy = torch.zeros(1, dtype=torch.float64, device=te.device)
    empty = torch.zeros((0, 3), dtype=torch.int32, device=te.device)
    ids1, ids2 = ops.to_ids(links[:, 0].copy()), ops.to_ids(links[:, 1].copy())
    work = None
    for _ in range(2):
        work = ops.mapping_step(te, d, True, ids1, ids2, tm, tma if opt == "Adagrad" else None, alpha, lr, opt, ws, n_ent, 3, loss, work)
        ops.triple_step(te, tea, rel, torch.full_like(rel, 0.1), d, empty, None, cfg, ws, dummy, phase=ops.PHASE_APPLY)
    assert abs(float(loss.item()) - ref_loss) <= 1e-5 * abs(ref_loss)
    assert np.linalg.norm(te[:, :d].cpu().numpy() - e0) <= 1e-4 * np.linalg.norm(e0)
    assert np.linalg.norm(tm.cpu().numpy() - m0) <= 1e-4 * np.linalg.norm(m0)
    assert int(ws[: -8 * 4096].count_nonzero()) == 0


def test_packed_tiles_bit_exact(ops):
    """The packed-operand (LDS-DMA) similarity tiles on ragged shapes: the similarity strip, the fused ranks / argmax
    (plain and CSLS) and the kNN sets are the oracle's bits (the same k-ordered fmaf chain)."""
    from oracle import cport
    rng = np.random.RandomState(5)
    for n1, n2, d in ((300, 517, 75), (129, 1000, 100), (640, 640, 300), (1, 130, 8)):
        e1 = rng.standard_normal((n1, d)).astype(np.float32)
        e2 = rng.standard_normal((n2, d)).astype(np.float32)
        t1, t2 = ops.to_table(e1), ops.to_table(e2)
        assert np.array_equal(ops.sim_matrix(t1, t2, d).cpu().numpy(), cport.sim_matrix(e1, e2, "inner"))
        if n1 <= n2:
            r, a = ops.rank_eval(t1, t2, d)
            r_ref, a_ref = cport.rank_eval(e1, e2, "inner")
            assert np.array_equal(r.cpu().numpy(), r_ref) and np.array_equal(a.cpu().numpy(), a_ref)
            cr, cc = rng.rand(n1).astype(np.float32), rng.rand(n2).astype(np.float32)
            r, a = ops.rank_eval(t1, t2, d, csls_r=torch.from_numpy(cr).cuda(), csls_c=torch.from_numpy(cc).cuda())
            r_ref, a_ref = cport.rank_eval(e1, e2, "inner", csls_r=cr, csls_c=cc)
            assert np.array_equal(r.cpu().numpy(), r_ref) and np.array_equal(a.cpu().numpy(), a_ref)
        k = min(37, n2)
        assert np.array_equal(ops.topk_inner(t1, t2, d, k).cpu().numpy(), cport.topk_inner(e1, e2, k))


@pytest.mark.parametrize("opt", ["Adam", "Adadelta"])
def test_triple_step_dense_optimisers_vs_oracle(ops, opt, capsys):
    """optimizers.py:13-16 through the fused step: the gradient w.r.t. the raw variables is the oracle's (read off one
    SGD step with lr = 1), the update is TF's dense Adam / Adadelta arithmetic on EVERY row (np_oracle.adam_tf)."""
    from _tol import assert_rows_close
    from oracle import cport, np_oracle as orc
    rng = np.random.RandomState(11)
    n_ent, n_rel, n_pos, k, d = 500, 17, 600, 4, 100
    ent = (rng.standard_normal((n_ent, d)) / np.sqrt(d)).astype(np.float32) * 1.2
    rel = (rng.standard_normal((n_rel, d)) / np.sqrt(d)).astype(np.float32)
    pos, neg = _kg(rng, n_ent, n_rel, n_pos, k)
    kw = dict(loss="limited", loss_norm="L2", pos_margin=0.01, neg_margin=2.0, balance=0.2)
    lr = 0.01 if opt == "Adam" else 0.5
    cfg = ops.make_step_cfg(neg_group_k=k, optimizer=opt, lr=lr, **kw)
    d_ent, d_rel = ops.to_table(ent), ops.to_table(rel)
    st_e = torch.zeros((2,) + tuple(d_ent.shape), device=d_ent.device)
    st_r = torch.zeros((2,) + tuple(d_rel.shape), device=d_ent.device)
    ws = ops.step_workspace(n_ent, n_rel, ops.pad4(d))
    loss_acc = torch.zeros(1, dtype=torch.float64, device=d_ent.device)
    ref = {"e": ent.astype(np.float64), "r": rel.astype(np.float64)}
    state = {kk: [np.zeros_like(v), np.zeros_like(v)] for kk, v in ref.items()}
    for t in range(1, 4):
        cfg.opt_t = t
        ops.triple_step(d_ent, st_e, d_rel, st_r, d, ops.to_ids(pos), ops.to_ids(neg), cfg, ws, loss_acc)
        e32, r32 = ref["e"].astype(np.float32), ref["r"].astype(np.float32)
        e1, r1 = e32.copy(), r32.copy()
        cport.triple_step(e1, None, r1, None, pos, neg, optimizer="SGD", lr=1.0, **kw)
        grads = {"e": e32.astype(np.float64) - e1, "r": r32.astype(np.float64) - r1}
        for kk in ("e", "r"):
            g, (s0, s1) = grads[kk], state[kk]
            if opt == "Adam":
                orc.adam_tf(ref[kk], g, s0, s1, lr, t)          # in place
            else:                                            # training_ops ApplyAdadelta, rho 0.95, eps 1e-8
                acc = s0 * 0.95 + g * g * 0.05
                upd = np.sqrt(s1 + 1e-8) / np.sqrt(acc + 1e-8) * g
                state[kk][0], state[kk][1] = acc, s1 * 0.95 + upd * upd * 0.05
                ref[kk] = ref[kk] - lr * upd
    with capsys.disabled():
        assert_rows_close(d_ent.cpu().numpy()[:, :d], ref["e"], "%s, entity table after 3 steps" % opt, tol=2e-4)
        assert_rows_close(d_rel.cpu().numpy()[:, :d], ref["r"], "%s, relation table after 3 steps" % opt, tol=2e-4)
    if opt == "Adam":
        assert float(np.abs(d_ent.cpu().numpy()[:, :d] - ent).max()) > 1e-3
    assert not bool((ws[: ws.numel() - 8 * 4096] != 0).any().item())


def test_adadelta_without_normalisation_is_sparse(ops):
    """ent_l2_norm / rel_l2_norm off: TF's gradient of the lookups is IndexedSlices and SparseApplyAdadelta visits the
    gathered rows only -- rows no triple of the batch touches keep their variable AND their accumulators."""
    rng = np.random.RandomState(12)
    n_ent, n_rel, n_pos, k, d = 400, 9, 50, 2, 32
    ent = (rng.standard_normal((n_ent, d)) / np.sqrt(d)).astype(np.float32)
    rel = (rng.standard_normal((n_rel, d)) / np.sqrt(d)).astype(np.float32)
    pos, neg = _kg(rng, 200, n_rel, n_pos, k)                   # entity ids < 200: rows 200.. are never gathered
    cfg = ops.make_step_cfg(neg_group_k=k, optimizer="Adadelta", lr=0.5, loss="limited", loss_norm="L2", pos_margin=0.01,
                            neg_margin=2.0, balance=0.2, ent_l2_norm=False, rel_l2_norm=False)
    d_ent, d_rel = ops.to_table(ent), ops.to_table(rel)
    st_e = torch.full((2,) + tuple(d_ent.shape), 0.25, device=d_ent.device)      # non-zero state: a dense pass would decay it
    st_r = torch.full((2,) + tuple(d_rel.shape), 0.25, device=d_ent.device)
    ws = ops.step_workspace(n_ent, n_rel, ops.pad4(d))
    loss_acc = torch.zeros(1, dtype=torch.float64, device=d_ent.device)
    for t in range(1, 3):
        cfg.opt_t = t
        ops.triple_step(d_ent, st_e, d_rel, st_r, d, ops.to_ids(pos), ops.to_ids(neg), cfg, ws, loss_acc)
    touched = np.zeros(n_ent, bool)
    touched[np.unique(np.concatenate([pos[:, [0, 2]].ravel(), neg[:, [0, 2]].ravel()]))] = True
    e_now, s_now = d_ent.cpu().numpy()[:, :d], st_e.cpu().numpy()[:, :, :d]
    assert np.array_equal(e_now[~touched], ent[~touched]) and np.all(s_now[:, ~touched] == 0.25)
    assert np.abs(e_now[touched] - ent[touched]).max() > 1e-4 and np.any(s_now[0][touched] != 0.25)


def test_dense_sgd_any_shape(ops):
    """DenseSGD (tf.train.GradientDescentOptimizer over dense parameters): 1-D biases, widths that are not a multiple of
    4 and non-contiguous views all take oea_sgd_rows."""
    from openea_amd.models.graph_ops import DenseSGD
    dev = ops.device()
    rng = np.random.RandomState(3)
    shapes = [(1000,), (37, 50), (300, 256), (5,)]
    params = [torch.tensor(rng.standard_normal(sh).astype(np.float32), device=dev, requires_grad=True) for sh in shapes]
    base = torch.tensor(rng.standard_normal((64, 48)).astype(np.float32), device=dev)
    view = base.t()                                         # non-contiguous parameter
    view.requires_grad_(True)
    params.append(view)
    before = [p.detach().cpu().numpy().copy() for p in params]
    grads = [rng.standard_normal(tuple(p.shape)).astype(np.float32) for p in params]
    for p, g in zip(params, grads):
        p.grad = torch.tensor(g, device=dev)
    DenseSGD(params, 0.3).step()
    for p, b, g in zip(params, before, grads):
        np.testing.assert_allclose(p.detach().cpu().numpy(), b - np.float32(0.3) * g, rtol=1e-6, atol=1e-7)
        assert p.grad is None


@pytest.mark.parametrize("case", ["random", "clusters", "ties"])
def test_topk_strip_free_path_bit_exact(ops, case, monkeypatch):
    """one table against itself at 33,000 rows: no similarity strip in HBM -- the stream form of the symmetric search
    (upper-triangle sweep, record streams, bucketing, list select); rows whose
    survivor lists overflow / fall short / are tie-heavy are redone by the fallback kernel.  All of it must equal the
    oracle's (value desc, column asc) selection bit for bit -- and the strip path (OEA_TOPK_LISTS=0 is read once per
    process, so the comparison with it is through the oracle)."""
    from oracle import cport
    rng = np.random.RandomState(7)
    n, d, k = 33000, 40, 700
    x = rng.standard_normal((n, d)).astype(np.float32)
    if case == "clusters":                       # 30 tight clusters in id order: whole candidate tiles survive for their members
        cen = rng.standard_normal((30, d)).astype(np.float32)
        x = cen[np.arange(n) * 30 // n] + 0.05 * x
    if case == "ties":                           # 3,000 identical rows: thousands of exact ties at the k-th value
        x[5000:8000] = x[5000]
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    t = ops.to_table(x)
    ids = ops.to_ids((np.arange(n, dtype=np.int32) * 3 + 1))
    out = ops.topk_inner(t, t, d, k, id_map=ids).cpu().numpy()
    assert out.shape == (n, k) and np.all(np.diff(out, axis=1) > 0)
    rows = np.concatenate([rng.choice(n, 40, replace=False), np.array([5000, 5001, 7999, 8000, 0, n - 1])])
    ref = cport.topk_inner(x[rows], x, k)
    assert np.array_equal(out[rows], ref * 3 + 1)


@pytest.mark.parametrize("d", [40, 75, 100])
def test_topk_stream_form_every_sweep_instance_equals_strip_path(ops, d):
    """the stream form's three sweep instances: d = 40 / 75 / 100 pack to Kp = 64 / 96 / 128, i.e. both operands through LDS, and
    the query operand in registers as 3 and 4 chunks.  12,400 rows is the form's smallest size band with a ragged last tile (112
    rows); duplicated rows tie inside one tile and across the first and the last.  A copy of the table as candidates takes
    the N x N strips (nc < 32,768): both must give the same sets on every row, and the oracle's on sampled rows."""
    from oracle import cport
    rng = np.random.RandomState(d)
    n, k = 12400, 250
    assert ops.lib().oea_topk_sym_workspace_bytes(n, k) > 0
    x = rng.standard_normal((n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x[5] = x[4]
    x[n - 1] = x[0]
    t = ops.to_table(x)
    sym = ops.topk_inner(t, t, d, k).cpu().numpy()
    strip = ops.topk_inner(t, t.clone(), d, k).cpu().numpy()
    assert np.array_equal(sym, strip)
    rows = np.concatenate([[0, 127, 128, 12287, 12288, n - 1], rng.choice(n, 12, replace=False)])
    assert np.array_equal(sym[rows], cport.topk_inner(x[rows], x, k))


@pytest.mark.parametrize("case", ["random", "clusters", "ties", "unnormalised", "d300_k10", "row_block"])
def test_topk_general_path_on_the_bf16_split_bit_exact(ops, case):
    """queries != candidates (batch.py:122-165 with a sub-list of entities; the bootstrapping candidates of alignment_finder.py:12-60;
    a rank's row block of a sharded refresh) at nc >= 32,768, nq >= 4,096: the threshold-append sweep runs on the bf16 hi / lo split
    of BOTH tables (round 6), the lists hold approximate values >= thr - tol, and the select decides the neighbourhood of the k-th
    value with exact k-ordered chains of the query row against the candidate rows.  The sets must be the oracle's (value desc,
    column asc), bit for bit: tight clusters (whole tiles survive), thousands of exact ties at the k-th value, rows of very
    different norms (the bound is on the largest), d = 300 with k = 10."""
    from oracle import cport
    rng = np.random.RandomState(11)
    nq, nc, d, k = (4300, 33000, 300, 10) if case == "d300_k10" else (4300, 33000, 40, 700)
    c = rng.standard_normal((nc, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    if case == "clusters":
        cen = rng.standard_normal((30, d)).astype(np.float32)
        c = cen[np.arange(nc) * 30 // nc] + 0.05 * c
        q = cen[np.arange(nq) * 30 // nq] + 0.05 * q
    if case == "ties":
        c[5000:8000] = c[5000]
        q[100:200] = c[5000]
    if case != "unnormalised":
        c /= np.linalg.norm(c, axis=1, keepdims=True)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
    else:
        c *= rng.uniform(0.1, 6.0, (nc, 1)).astype(np.float32)
        q *= rng.uniform(0.1, 6.0, (nq, 1)).astype(np.float32)
    if case == "row_block":                      # a rank's block of the table itself (models/dist.py:sharded_neighbours): every row finds itself
        q = c[5000:5000 + nq].copy()
    tq, tc = ops.to_table(q), ops.to_table(c)
    if case == "row_block":
        tq = tc[5000:5000 + nq]
    ids = ops.to_ids((np.arange(nc, dtype=np.int32) * 3 + 1))
    out = ops.topk_inner(tq, tc, d, k, id_map=ids).cpu().numpy()
    assert out.shape == (nq, k) and np.all(np.diff(out, axis=1) > 0)
    rows = np.concatenate([rng.choice(nq, 40, replace=False), np.array([100, 150, 199, 200, 0, nq - 1])])
    ref = cport.topk_inner(q[rows], c, k)
    assert np.array_equal(out[rows], ref * 3 + 1)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("case", ["random", "duplicates", "constant", "unnormalised", "alinet1200", "d500"])
def test_csls_means_one_sweep_bit_exact(ops, case, bf16, monkeypatch):
    """oea_csls_means (thresholded one-sweep lists + fallbacks) == row_topk_mean over the strips of S and S^T, bit for
    bit, also when duplicate rows overflow lists or a constant matrix sends every row through the fallbacks.  bf16: the sweep
    multiplies the hi / lo split (the product path from 3e8 pairs on; forced here), the lists hold approximate values with the
    index of the other side and the means are taken over the exact chains of the entries that can belong to the top k."""
    monkeypatch.setenv("OEA_CSLS_BF16_MIN_PAIRS", "1" if bf16 else "1e30")
    rng = np.random.RandomState(21)
    n1, n2, d, k = {"random": (10500, 10500, 75, 10), "alinet1200": (4200, 4400, 1200, 10), "d500": (4100, 4300, 500, 10)}.get(case, (4300, 4700, 32, 10))
    e1 = rng.standard_normal((n1, d)).astype(np.float32)
    e2 = rng.standard_normal((n2, d)).astype(np.float32)
    if case == "alinet1200":             # AliNet's evaluation rows: three L2-normalised blocks side by side (alinet.py:948-966), norm sqrt(3)
        e2[:n1] = e1 + 0.7 * e2[:n1]
        for lo, hi in ((0, 500), (500, 900), (900, 1200)):
            e1[:, lo:hi] /= np.linalg.norm(e1[:, lo:hi], axis=1, keepdims=True)
            e2[:, lo:hi] /= np.linalg.norm(e2[:, lo:hi], axis=1, keepdims=True)
    if case == "duplicates":
        e2[1000:1900] = e2[1000]                 # 900 identical candidates: their column lists and the rows near them overflow
        e1[10:60] = e1[10]
    if case == "constant":
        e1[:] = e1[0]
        e2[:] = e2[0]
    e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
    e2 /= np.linalg.norm(e2, axis=1, keepdims=True)
    if case == "unnormalised":
        e1 = (e1 * rng.uniform(0.2, 3.0, (n1, 1))).astype(np.float32)
        e2 = (e2 * rng.uniform(0.2, 3.0, (n2, 1))).astype(np.float32)
    t1, t2 = ops.to_table(e1), ops.to_table(e2)
    got = ops.csls_means(t1, t2, d, k)
    assert got is not None
    r, c = got
    r_ref = ops.row_topk_mean(ops.sim_matrix(t1, t2, d, "inner"), k)
    c_ref = ops.row_topk_mean(ops.sim_matrix(t2, t1, d, "inner"), k)
    assert torch.equal(r, r_ref) and torch.equal(c, c_ref)


@pytest.mark.parametrize("m,k1,k2", [(5000, 300, 300), (70001, 500, 400), (33, 8, 12), (4097, 400, 300), (20000, 128, 64), (1000, 6, 8)])
def test_gemm_tn_matches_float64(ops, m, k1, k2):
    """dW = X^T dY of the GNN dense layers (alinet.py:574-582, rdgcn.py:250-256) on the fp32 matrix cores with the row
    reduction split into chunks: against a float64 product (fp32 accumulation error only), two runs bit-identical, and the
    autograd wrapper's three gradients against torch's."""
    import torch
    from openea_amd.models.graph_ops import dense
    dev = ops.device()
    g = torch.Generator(device=dev).manual_seed(m)
    a = torch.randn(m, k1, device=dev, generator=g)
    b = torch.randn(m, k2, device=dev, generator=g)
    got = ops.gemm_tn(a, b)
    assert torch.equal(got, ops.gemm_tn(a, b))
    ref = a.double().t() @ b.double()
    assert got.shape == ref.shape
    err = (got.double() - ref).abs().max().item()
    assert err <= 2e-6 * (m ** 0.5) * 4 + 1e-5, err
    lib_err = ((a.t() @ b).double() - ref).abs().max().item()
    assert err <= 10 * lib_err + 1e-4, (err, lib_err)                   # the same order as the library's own rounding
    x = a.clone().requires_grad_(True)
    w = (torch.randn(k1, k2, device=dev, generator=g) * 0.1).requires_grad_(True)
    bias = torch.randn(k2, device=dev, generator=g).requires_grad_(True)
    (dense(x, w, bias) * b).sum().backward()
    x2, w2, bias2 = a.clone().requires_grad_(True), w.detach().clone().requires_grad_(True), bias.detach().clone().requires_grad_(True)
    (torch.addmm(bias2, x2, w2) * b).sum().backward()
    assert torch.allclose(x.grad, x2.grad, rtol=1e-5, atol=1e-5)
    assert (w.grad - w2.grad).abs().max().item() <= 1e-5 * max(w2.grad.abs().max().item(), 1.0) * 8
    assert torch.allclose(bias.grad, bias2.grad, rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("case", ["random", "trained", "clustered", "ties", "degenerate", "outliers"])
def test_manhattan_evaluation_from_grid_distances_equals_all_pairs_fp64(ops, case, monkeypatch):
    """RDGCN's evaluation metric (similarity.py:46-48, alignment.py:146-168): ranks and nearest candidates from 16-bit grid
    distances + exact similarities where the grid leaves a doubt == the all-pairs fp64 kernel (itself bit-exact with scipy's
    cdist, tests above), on random rows, rows whose gold is the nearest ('trained'), tight clusters (hundreds of candidates
    within the grid's error of the gold distance), exact duplicates of gold columns (the tie rule), a table of identical
    rows (every list overflows: the in-kernel all-pairs path) and a table with two huge outliers (the grid is useless: the
    first block goes exact in the kernel, the rest through the all-pairs kernel); a second block size exercises row0 > 0
    and a gold offset."""
    import torch
    rng = np.random.RandomState(11)
    n1, n2, d = 1500, 4000, 75
    e2 = rng.standard_normal((n2, d)).astype(np.float32) * 0.3
    off = 700
    if case == "random":
        e1 = rng.standard_normal((n1, d)).astype(np.float32) * 0.3
    elif case == "trained":
        e1 = e2[off:off + n1] + 0.05 * rng.standard_normal((n1, d)).astype(np.float32)
    elif case == "clustered":
        e2[1000:3000] = e2[1000] + 2e-4 * rng.standard_normal((2000, d)).astype(np.float32)
        e1 = e2[off:off + n1] + 1e-4 * rng.standard_normal((n1, d)).astype(np.float32)
    elif case == "ties":
        e1 = e2[off:off + n1] + 0.02 * rng.standard_normal((n1, d)).astype(np.float32)
        e2[3000:3400] = e2[off:off + 400]                          # exact copies of gold columns behind them
        e2[0:300] = e2[off + 500:off + 800]                        # ... and in front of them
    elif case == "outliers":                                       # two huge entries stretch the grid: its error bound exceeds every
        e1 = e2[off:off + n1] + 0.05 * rng.standard_normal((n1, d)).astype(np.float32)     # distance, whole rows go exact and the
        e2[5, 3], e2[3999, 70] = 4000.0, -4000.0                   # caller leaves the grid after the first block of rows
    else:
        e2[:] = e2[0]
        e1 = np.repeat(e2[:1], n1, axis=0)
    t1, t2 = ops.to_table(e1), ops.to_table(e2)
    monkeypatch.setenv("OEA_L1_EVAL", "f64")
    ref_rank, ref_arg = ops.rank_eval(t1, t2, d, "manhattan", gold_offset=off)
    monkeypatch.setenv("OEA_L1_EVAL", "grid")
    rank, arg = ops.rank_eval(t1, t2, d, "manhattan", gold_offset=off)
    assert torch.equal(rank, ref_rank) and torch.equal(arg, ref_arg)
    rank, arg = ops.rank_eval_l1_grid(t1, t2, d, gold_offset=off, block_bytes=4 * 4000 * 600)     # three blocks of rows
    assert torch.equal(rank, ref_rank) and torch.equal(arg, ref_arg)
    if case == "trained":
        assert int((rank == 0).sum()) > n1 // 2
    # ---- the same with CSLS (basic_model.py:132-135: test() evaluates a second time with csls = args.csls): the means from
    # the k + margin nearest on the grid (certified lists, exact similarities in scipy's summation order) and the ranks of
    # (2 s - r) - c from the strip + exact decisions == strips of every pair in fp64 + rank_valu_kernel
    from openea_amd.modules.finding.similarity import csls_means_device
    sq = e2[off:off + n1] + 0.05 * rng.standard_normal((n1, d)).astype(np.float32) if case in ("random",) else e1
    s1, s2 = ops.to_table(sq), t2
    k = 10
    monkeypatch.setenv("OEA_L1_EVAL", "f64")
    r_ref, c_ref = csls_means_device(s1, s2, d, "manhattan", k)
    rk_ref, am_ref = ops.rank_eval(s1, s2, d, "manhattan", r_ref, c_ref, gold_offset=off)
    monkeypatch.setenv("OEA_L1_EVAL", "grid")
    stats = {}
    grid = ops.L1Grid(s1, s2, d, block_bytes=4 * 4000 * 600)
    r = ops.l1_grid_topk_means(s1, s2, grid.q1, grid.q2, d, k, grid.step, grid.err, keep=grid, stats=stats)
    c = ops.l1_grid_topk_means(s2, s1, grid.q2, grid.q1, d, k, grid.step, grid.err, block_bytes=4 * 1500 * 1000, stats=stats)
    assert torch.equal(r, r_ref) and torch.equal(c, c_ref), (case, stats)
    assert len(grid.strips) == 3                                   # left behind for the rank pass
    rk, am = ops.rank_eval_l1_grid(s1, s2, d, gold_offset=off, csls_r=r, csls_c=c, grid=grid)
    assert torch.equal(rk, rk_ref) and torch.equal(am, am_ref), case
    assert not grid.strips
    rk, am = ops.rank_eval(s1, s2, d, "manhattan", r, c, gold_offset=off)        # the dispatch (fresh grid, default blocks)
    assert torch.equal(rk, rk_ref) and torch.equal(am, am_ref)
    if case in ("degenerate", "outliers", "clustered"):
        assert stats["uncertified"] > 0                             # these tables send rows through the all-pairs fallback
    else:
        # a numpy replay of the certificate (tests/test_l1_grid_gpu.py:restate_topk_means_uncertified) finds no row of either
        # direction uncertified on these three tables (grid distances within 19 of the 77.5 steps L1Grid.err allows): the lists
        # must carry the means, not the fallback
        assert stats["uncertified"] == 0, (case, stats)


WAVE_WORKER = r'''
import os, sys
import numpy as np
import torch
sys.path.insert(0, os.environ["OEA_ROOT"])
from openea_amd import ops
assert ops.deterministic()
out = {}
for d, n_pos, k, sides in ((100, 6500, 10, "same"), (75, 5000, 10, "same"), (37, 4100, 7, "mixed"), (128, 3000, 3, "same"), (200, 2000, 10, "same")):
    rng = np.random.RandomState(d)
    n_ent, n_rel = 5000, 61
    ent0 = (rng.standard_normal((n_ent, d)) / np.sqrt(d)).astype(np.float32) * 1.3
    rel0 = (rng.standard_normal((n_rel, d)) / np.sqrt(d)).astype(np.float32) * 0.7
    w = 1.0 / np.arange(1, n_ent + 1) ** 0.9
    pos = np.stack([rng.choice(n_ent, n_pos, p=w / w.sum()), rng.randint(0, n_rel, n_pos), rng.randint(0, n_ent, n_pos)], 1).astype(np.int32)
    neg = np.repeat(pos, k, 0)
    # the sampler corrupts ONE side per round (batch.py:101-107): all k negatives of a positive on one side ("same"), or
    # a side per negative ("mixed": rounds after a collision) -- the wave kernel's fast and independent-triple paths
    flip = np.repeat(rng.rand(n_pos) < 0.5, k) if sides == "same" else rng.rand(len(neg)) < 0.5
    neg[flip, 0] = rng.randint(0, n_ent, int(flip.sum()))
    neg[~flip, 2] = rng.randint(0, n_ent, int((~flip).sum()))
    neg[5] = (3, 1, 4)                      # an entry that is NOT a corruption of its positive
    neg[3 * k] = pos[3]                     # a negative equal to its positive (max_try exhausted)
    e, r = ops.to_table(ent0), ops.to_table(rel0)
    ea, ra = torch.full_like(e, 0.1), torch.full_like(r, 0.1)
    ws = ops.step_workspace(n_ent, n_rel, ops.pad4(d))
    loss = torch.zeros(1, dtype=torch.float64, device=e.device)
    cfg = ops.make_step_cfg(loss="limited", loss_norm="L2" if d != 37 else "L1", pos_margin=0.01, neg_margin=2.0, balance=0.2, optimizer="Adagrad",
                            lr=0.01, neg_group_k=k)
    for _ in range(3):
        ops.triple_step(e, ea, r, ra, d, ops.to_ids(pos), ops.to_ids(neg), cfg, ws, loss)
    torch.cuda.synchronize()
    out["e%d" % d], out["r%d" % d], out["l%d" % d] = e.cpu().numpy(), r.cpu().numpy(), float(loss.item())
np.savez(os.environ["OEA_OUT"], **out)
'''


def test_wave_per_positive_step_kernel_equals_the_grouped_kernel(tmp_path):
    """triple_wave (one wave per positive: scalar ids, buffer addressing, one accumulator for the two rows that receive the same
    sum) against triple_grouped (OEA_STEP_WAVE=0: two positives per wave) in the fixed-point build, where the scatter-add has no
    order: three Adagrad steps on Zipf-headed batches (d = 100 / 75 / 128 / 200 with every positive's negatives on one side --
    the select-free loops; d = 37 with the L1 norm and a side per negative -- the independent-triple path; an entry that is no
    corruption of its positive; a negative equal to its positive).  The two kernels reduce a row over 64 / 32 lanes, so a score
    differs in its last bit and the tables agree to 1e-6 of their norm, not bit for bit; run to run each kernel IS bit-stable."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for tag, wave in (("g", "0"), ("w", "1"), ("w2", "1")):
        out = str(tmp_path / ("wave%s.npz" % tag))
        env = dict(os.environ, OEA_ROOT=root, OEA_OUT=out, OEA_STEP_DETERMINISTIC="1", OEA_STEP_WAVE=wave)
        p = subprocess.run([sys.executable, "-c", WAVE_WORKER], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        assert p.returncode == 0, p.stdout.decode(errors="replace")[-3000:]
        res[tag] = dict(np.load(out))
    # the oracle on the same batches: which kernel is off, should the two disagree
    from oracle import cport
    worst = {}
    for d, n_pos, k, sides in ((100, 6500, 10, "same"), (75, 5000, 10, "same"), (37, 4100, 7, "mixed"), (128, 3000, 3, "same"), (200, 2000, 10, "same")):
        rng = np.random.RandomState(d)
        n_ent, n_rel = 5000, 61
        ent = (rng.standard_normal((n_ent, d)) / np.sqrt(d)).astype(np.float32) * 1.3
        rel = (rng.standard_normal((n_rel, d)) / np.sqrt(d)).astype(np.float32) * 0.7
        w = 1.0 / np.arange(1, n_ent + 1) ** 0.9
        pos = np.stack([rng.choice(n_ent, n_pos, p=w / w.sum()), rng.randint(0, n_rel, n_pos), rng.randint(0, n_ent, n_pos)], 1).astype(np.int32)
        neg = np.repeat(pos, k, 0)
        flip = np.repeat(rng.rand(n_pos) < 0.5, k) if sides == "same" else rng.rand(len(neg)) < 0.5
        neg[flip, 0] = rng.randint(0, n_ent, int(flip.sum()))
        neg[~flip, 2] = rng.randint(0, n_ent, int((~flip).sum()))
        neg[5] = (3, 1, 4)
        neg[3 * k] = pos[3]
        ea, ra = np.full_like(ent, 0.1), np.full_like(rel, 0.1)
        for _ in range(3):
            cport.triple_step(ent, ea, rel, ra, pos, neg, loss="limited", loss_norm="L2" if d != 37 else "L1", pos_margin=0.01, neg_margin=2.0,
                              balance=0.2, optimizer="Adagrad", lr=0.01)
        for tag in ("g", "w"):
            dev = np.linalg.norm(res[tag]["e%d" % d][:, :d] - ent, axis=1)
            worst[(tag, d)] = (float(dev.max()), int(dev.argmax()), int((dev > 1e-4).sum()))
    bad = {kk: v for kk, v in worst.items() if v[0] > 2e-4}
    assert not bad, "rows off the oracle by more than 2e-4 (kernel g = triple_grouped, w = triple_wave; max deviation, row, rows > 1e-4): %s" % bad
    for d in (100, 75, 37, 128, 200):
        for t in ("e", "r"):
            a, b = res["g"]["%s%d" % (t, d)], res["w"]["%s%d" % (t, d)]
            assert np.linalg.norm(a - b) <= 1e-6 * np.linalg.norm(a), (t, d, np.linalg.norm(a - b) / np.linalg.norm(a), worst)
            assert np.array_equal(b, res["w2"]["%s%d" % (t, d)]), (t, d)          # fixed-point sums: the same bits run to run
        la, lb = float(res["g"]["l%d" % d]), float(res["w"]["l%d" % d])
        assert abs(la - lb) <= 1e-6 * abs(la), d


@pytest.mark.parametrize("k", [10, 3, 1])
def test_step_plan_equals_the_oracle_restatement(ops, k):
    """oea_step_plan_build (the (step, row)-sorted references of an epoch's positives: which entity row adds which positive's
    gradient rows, with which sign, in batch order) against oracle/np_oracle.py:step_plan on an epoch of ragged batches (one of
    them empty) whose negatives are mostly one-sided per positive -- the sampler's output -- with positives of mixed sides, a
    foreign entry, a negative equal to its positive and self-loops in between."""
    from oracle import np_oracle
    rng = np.random.RandomState(40 + k)
    n_ent, n_rel, ld = 3000, 17, 36
    sizes = [700, 0, 1333, 64, 901]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offsets[-1])
    pos = np.stack([rng.randint(0, n_ent, n), rng.randint(0, n_rel, n), rng.randint(0, n_ent, n)], 1).astype(np.int32)
    pos[7, 2] = pos[7, 0]                                            # a self-loop: both references on one row
    pos[800:840, 0] = 42                                             # a hub of step 2: 40 heads on one row (+ 30 tails on another)
    pos[850:880, 2] = 77
    neg = np.repeat(pos, k, 0)
    side = np.repeat(rng.rand(n) < 0.5, k)
    mixed = np.repeat(rng.rand(n) < 0.05, k)                         # rounds after a collision: a side per negative
    side = np.where(mixed, rng.rand(n * k) < 0.5, side)
    neg[side, 0] = rng.randint(0, n_ent, int(side.sum()))
    neg[~side, 2] = rng.randint(0, n_ent, int((~side).sum()))
    neg[5 * k] = (3, 1, 4)                                           # not a corruption of positive 5
    neg[9 * k: 10 * k] = pos[9]                                      # negatives equal to their positive (max_try exhausted)
    dev = ops.device()
    d_pos, d_neg = ops.to_ids(pos), ops.to_ids(neg)
    off_dev = torch.from_numpy(offsets).to(dev)
    dims = (n, len(sizes), max(sizes), n_ent, ld)
    plan = ops.step_plan_buffer(*dims, dev=dev)
    ops.step_plan_build(d_pos, d_neg, k, off_dev, *dims, plan)
    torch.cuda.synchronize()
    got = ops.step_plan_arrays(plan, *dims)
    ref = np_oracle.step_plan(pos, neg, k, offsets, n_ent)
    assert got["row_bits"] == ref["row_bits"]
    nu = len(ref["ukeys"])
    sf = got["step_first"]
    assert np.array_equal(sf, ref["step_first"])                      # (the last entry = number of keys of real steps)
    assert np.array_equal(got["ukeys"][:nu], ref["ukeys"])
    assert np.array_equal(got["uoff"][:nu + 1], ref["uoff"])
    assert np.array_equal(got["vals"][:len(ref["vals"])], ref["vals"])
    assert 0 < nu <= 2 * n and sf[1] == sf[2]                         # the empty batch owns no keys
    assert np.array_equal(got["pflags"], ref["pflags"])
    assert (ref["pflags"][800:840] & 1).sum() >= 38 and (ref["pflags"][850:880] & 2).sum() >= 28      # (mixed-side positives drop out)


PLAN_WORKER = r'''
import os, sys
import numpy as np
import torch
sys.path.insert(0, os.environ["OEA_ROOT"])
from openea_amd import ops
from openea_amd.models.trainer import EmbeddingTable, RelationTripleEpochs, TripleTrainer, refresh_neighbours
from openea_amd.modules.base.initializers import truncated_normal_host
from openea_amd.modules.load.synth import make_kgs
dev = torch.device("cuda", 0)
out = {}
for d, k, B, norm in ((32, 10, 1500, "L2"), (75, 5, 2600, "L1"), (100, 10, 900, "L2")):
    kgs = make_kgs("small", mode="swapping", seed=1)
    rng = np.random.RandomState(d)
    ent_h = truncated_normal_host(rng, (kgs.entities_num, d), 1.0 / np.sqrt(d))
    ent, ent0 = EmbeddingTable(ent_h, True, "ent_embeds", dev), EmbeddingTable(ent_h.copy(), True, "ent_embeds_0", dev)
    rel = EmbeddingTable(truncated_normal_host(rng, (kgs.relations_num, d), 1.0 / np.sqrt(d)), True, "rel_embeds", dev)
    cfg = ops.make_step_cfg(loss="limited", loss_norm=norm, pos_margin=0.01, neg_margin=2.0, balance=0.2, optimizer="Adagrad", lr=0.01,
                            neg_group_k=k)
    tr = TripleTrainer(ent, rel, cfg, "Adagrad")
    ep = RelationTripleEpochs(kgs, B, k, seed=11, dev=dev)
    S = len(ep.batches.splits)
    assert ops.step_plan_supported(cfg, ent.rows, rel.rows, ent.ld, k) == (os.environ["OEA_STEP_PLAN"] == "2")
    n = ep.run_epoch(tr)                                   # epoch 1: negatives drawn and plan sorted inside the call
    n += ep.run_steps(tr, S + 2)                           # epoch 2 (prepared on the side stream) and two steps of epoch 3
    # (neighbour lists from the INITIAL table: lists from the trained one would turn last-bit differences of the two runs' fp32
    #  sums into different neighbour sets, different negatives and tables 1e-4 apart -- measured, six runs of ONE build)
    nbr = [refresh_neighbours(ent0, kg.entities_list, max(2, int(0.1 * kg.entities_num))) for kg in (kgs.kg1, kgs.kg2)]
    ep.set_neighbours(*nbr)                                # truncated sampling: the prepared negatives and plans are dropped
    n += ep.run_steps(tr, S - 2)                           # the rest of epoch 3: sampled step by step, no plan
    n += ep.run_steps(tr, 2 * S)                           # epochs 4 and 5 on new negatives
    ep.check()
    torch.cuda.synchronize()
    out["e%d" % d], out["r%d" % d], out["l%d" % d], out["n%d" % d] = ent.raw(), rel.raw(), tr.pop_loss(), n
np.savez(os.environ["OEA_OUT"], **out)
'''


def test_planned_epochs_equal_the_atomic_epochs(tmp_path):
    """Five epochs through the device epoch engine with the gathered-sum plan (the default: positives' own rows by plain stores +
    an ordered gather in the optimiser) against OEA_STEP_PLAN=0 (every gradient row through the atomic scratch): whole epochs,
    ranges that cross epoch boundaries (the plan of the next epoch is sorted on the side stream), a neighbour refresh in the
    middle of an epoch (prepared negatives and plan dropped, the rest of that epoch sampled step by step).  The two differ in the
    ORDER of fp32 additions only: tables within 2e-6 of their norm, loss within 1e-6.
    (Planned against atomic, never against the oracle, and with 32-lane groups only: tests/test_step_plan_gpu.py compares the planned
    step with the oracle in every dispatch.)"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for plan in ("2", "0"):                                  # 2: the plan whatever the table size (the default keeps it for tables > 128 MB)
        out = str(tmp_path / ("plan%s.npz" % plan))
        env = dict(os.environ, OEA_ROOT=root, OEA_OUT=out, OEA_STEP_PLAN=plan)
        env.pop("OEA_STEP_DETERMINISTIC", None)
        p = subprocess.run([sys.executable, "-c", PLAN_WORKER], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
        assert p.returncode == 0, p.stdout.decode(errors="replace")[-3000:]
        res[plan] = dict(np.load(out))
    for d in (32, 75, 100):
        assert int(res["2"]["n%d" % d]) == int(res["0"]["n%d" % d])
        for t in ("e", "r"):
            a, b = res["0"]["%s%d" % (t, d)], res["2"]["%s%d" % (t, d)]
            assert np.linalg.norm(a - b) <= 2e-6 * np.linalg.norm(a), (t, d, np.linalg.norm(a - b) / np.linalg.norm(a))
        la, lb = float(res["0"]["l%d" % d]), float(res["2"]["l%d" % d])
        assert abs(la - lb) <= 1e-6 * abs(la), d


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("n,c,k,largest", [(300, 42, 10, True), (257, 157, 125, False), (5, 1, 1, True), (64, 1024, 37, False), (100, 65, 65, True)])
def test_row_rank_select_equals_a_stable_sort(ops, dtype, n, c, k, largest):
    """oea_row_rank_select_*: the k best of every row of a short candidate matrix by ranking (ties to the earlier column), the
    selected columns in ascending order (mapped through an id list) and the k-th best value == a stable sort (what np.argsort /
    np.partition give on the candidate lists of get_neg, approaches/rdgcn.py:75-87, and of calculate_nearest_k,
    similarity.py:80-83); rows full of ties included."""
    rng = np.random.RandomState(n + c)
    v = rng.standard_normal((n, c))
    v[:, ::3] = np.round(v[:, ::3], 1)                                  # ties
    v[0] = 1.0
    v = v.astype(np.float32 if dtype == "f32" else np.float64)
    ids = np.sort(rng.choice(100000, (n, c), replace=True), axis=1).astype(np.int32)
    dv = torch.from_numpy(v).to(ops.device())
    sel, kth = ops.row_rank_select(dv, k, largest, ids=torch.from_numpy(ids).to(ops.device()), want_kth=True)
    order = np.argsort(-v if largest else v, axis=1, kind="stable")[:, :k]
    cols = np.sort(order, axis=1)
    assert np.array_equal(sel.cpu().numpy(), np.take_along_axis(ids, cols, 1))
    assert np.array_equal(kth.cpu().numpy(), np.take_along_axis(v, order[:, k - 1:k], 1).reshape(-1))
    sel2, _ = ops.row_rank_select(dv, k, largest)
    assert np.array_equal(sel2.cpu().numpy(), cols)


def test_epoch_layout_is_a_fresh_permutation_of_each_list(ops):
    """oea_epoch_layout (basic_model.py:234-235 random.shuffle of both KGs' lists + batch.py:17-22 batch layout): every epoch's
    layout visits each list's triples at most once and exactly as many as the layout has slots for that list, KG1's slice in front
    of KG2's in every batch; the same (seed, epoch) gives the same layout, another epoch another one; positions are uniform
    (a triple's mean slot over 64 epochs is near the middle)."""
    from openea_amd.modules.train.batch import EpochBatches
    from oracle import np_oracle as orc
    rng = np.random.RandomState(3)
    t1 = np.stack([rng.randint(0, 500, 4000), rng.randint(0, 9, 4000), np.arange(4000)], 1).astype(np.int32)       # unique by column 2
    t2 = np.stack([rng.randint(500, 900, 2500), rng.randint(0, 9, 2500), np.arange(4000, 6500)], 1).astype(np.int32)
    b = EpochBatches(t1, t2, 1000)
    gen = torch.Generator(device=ops.device())
    gen.manual_seed(17)
    first = b.dall.cpu().numpy().copy()
    assert np.array_equal(first, np.concatenate([t1, t2])[b.slot.cpu().numpy()])          # before any shuffle: the lists as loaded
    layouts, pos_sum = [], np.zeros(6500)
    for e in range(64):
        b.shuffle(gen)
        d = b.dall.cpu().numpy()
        layouts.append(d.copy())
        ids = d[:, 2]
        assert len(np.unique(ids)) == len(ids)                                              # nothing visited twice
        for s in range(len(b.splits)):
            o0, o1, sp = int(b.offsets[s]), int(b.offsets[s + 1]), int(b.splits[s])
            assert (ids[o0:o0 + sp] < 4000).all() and (ids[o0 + sp:o1] >= 4000).all()      # KG1's slice, then KG2's
        pos_sum[ids] += np.arange(len(ids))
        full = np.concatenate([t1, t2])
        assert np.array_equal(d, full[ids])                                                 # rows travel whole
        if e < 4:                                                                           # the keyed permutation, restated in numpy
            assert np.array_equal(d, orc.epoch_layout(t1, t2, b.slot.cpu().numpy(), 17, e + 1))
    assert not np.array_equal(layouts[0], layouts[1])
    b2 = EpochBatches(t1, t2, 1000)
    b2.shuffle(gen)
    assert np.array_equal(b2.dall.cpu().numpy(), layouts[0])                                # same seed, same epoch counter
    visited = pos_sum > 0
    mean_pos = pos_sum[visited] / 64
    assert abs(mean_pos[:100].mean() / len(first) - 0.5) < 0.12                              # no triple keeps to one end of the epoch
