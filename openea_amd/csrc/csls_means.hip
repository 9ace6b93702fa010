// csls_means.hip -- the CSLS terms of the reference's csls_sim (modules/finding/similarity.py:57-83): r_i / c_j = mean of the k
// largest similarities of row i / column j of S = e1 e2^T.
//
// This file holds: the per-row top-k mean on an explicit block of S (oea_row_topk_mean) and the correction itself
// (oea_csls_apply); the means of ALL rows and columns in one tile sweep that never writes S (oea_csls_means: sampled thresholds,
// csls_append_kernel on the fp32 or bf16 split pipelines of sim_tiles.h, the exact means from the survivor lists, fallbacks for
// rows whose list failed) with its plan and workspace layout.
#include "sim_tiles.h"
#include <stdlib.h>
#include <cmath>

using namespace oea;

namespace {

// ---- per-row top-k mean (CSLS) -------------------------------------------------------------------
// One wave per row, k <= 32.  Pass 1: every lane takes the maximum of its strided slice; the k-th largest of
// the 64 lane maxima is a lower bound L of the row's k-th largest value (they are k distinct entries >= L).
// Pass 2 (the row is L2-hot): the handful of entries >= L -- about k of them -- go to an LDS list.  The k
// largest of the list are then taken by k rounds of wave-wide "largest head" and summed in DESCENDING order
// exactly like oracle_topk_mean.  Rows with more than kCandMean entries >= L (constant / heavily tied rows)
// fall back to per-lane sorted insertion lists (the previous algorithm).
constexpr int kCandMean = 256;

template <int KMAX>
__device__ float topk_mean_by_insertion(const float *__restrict__ src, int64_t n2, int k, int lane) {
    float top[KMAX];
#pragma unroll
    for (int p = 0; p < KMAX; ++p) top[p] = -INFINITY;
    for (int64_t j = lane; j < n2; j += 64) {
        float v = src[j];
        if (v > top[KMAX - 1]) {
#pragma unroll
            for (int p = 0; p < KMAX; ++p) {
                const float hi = fmaxf(top[p], v), lo = fminf(top[p], v);
                top[p] = hi; v = lo;
            }
        }
    }
    float acc = 0.f;
    int taken = 0;    // how many of this lane's list were consumed
    for (int round = 0; round < k; ++round) {
        float head = -INFINITY;
#pragma unroll
        for (int p = 0; p < KMAX; ++p) if (p == taken) head = top[p];
        float m = head;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
        const unsigned long long bal = __ballot(head == m);      // lowest lane holding the maximum advances
        const int winner = __ffsll((long long)bal) - 1;
        if (lane == winner) ++taken;
        acc += m;
    }
    return acc / (float)k;
}

__global__ __launch_bounds__(256) void row_topk_mean_kernel(const float *__restrict__ s, int64_t n1, int64_t n2,
                                                            int64_t ld, int k, float *__restrict__ out,
                                                            const int32_t *__restrict__ out_index /* may be NULL */,
                                                            const int32_t *__restrict__ n_active /* may be NULL */) {
    __shared__ float s_cand[4][kCandMean];
    __shared__ int s_cnt[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * 4 + wave;
    if (row >= n1 || (n_active && row >= *n_active)) return;  // whole waves leave: no block-wide barrier below
    const float *src = s + row * ld;
    const bool vec = ((ld & 3) == 0) && ((reinterpret_cast<uintptr_t>(s) & 15) == 0);
    const int64_t n4 = vec ? (n2 & ~(int64_t)3) : 0;        // [0, n4) by float4, the rest scalar
    // ---- pass 1: lane maxima -> L ------------------------------------------------------------------
    float mx = -INFINITY;
    constexpr int U = 4;                                     // 16-byte loads in flight per lane
    for (int64_t j0 = (int64_t)lane * 4; j0 < n4; j0 += 256 * U) {
        float4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t j = j0 + u * 256;
            v[u] = j < n4 ? *reinterpret_cast<const float4 *>(src + j) : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) mx = fmaxf(fmaxf(mx, fmaxf(v[u].x, v[u].y)), fmaxf(v[u].z, v[u].w));
    }
    for (int64_t j = n4 + lane; j < n2; j += 64) mx = fmaxf(mx, src[j]);
    float head = mx, L = -INFINITY;
    for (int round = 0; round < k; ++round) {                // k <= 64 distinct lanes exist only if n2 >= 64 * ...; else L = -inf
        float m = head;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
        const unsigned long long bal = __ballot(head == m);
        if (lane == __ffsll((long long)bal) - 1) head = -INFINITY;
        L = m;
    }
    // ---- pass 2: entries >= L -----------------------------------------------------------------------
    if (lane == 0) s_cnt[wave] = 0;
    __builtin_amdgcn_wave_barrier();
    float *cand = s_cand[wave];
    for (int64_t j0 = (int64_t)lane * 4; j0 < n4; j0 += 256 * U) {
        float4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t j = j0 + u * 256;
            v[u] = j < n4 ? *reinterpret_cast<const float4 *>(src + j) : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (j0 + u * 256 >= n4) continue;
            const float vv[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (vv[q] >= L) { const int at = atomicAdd(&s_cnt[wave], 1); if (at < kCandMean) cand[at] = vv[q]; }
        }
    }
    for (int64_t j = n4 + lane; j < n2; j += 64) {
        const float v = src[j];
        if (v >= L) { const int at = atomicAdd(&s_cnt[wave], 1); if (at < kCandMean) cand[at] = v; }
    }
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
    const int cnt = s_cnt[wave];
    float result;
    if (cnt > kCandMean || cnt < k) {                        // wave-uniform
        result = k <= 16 ? topk_mean_by_insertion<16>(src, n2, k, lane) : topk_mean_by_insertion<32>(src, n2, k, lane);
    } else {
        float c[kCandMean / 64];
#pragma unroll
        for (int u = 0; u < kCandMean / 64; ++u) c[u] = (u * 64 + lane) < cnt ? cand[u * 64 + lane] : -INFINITY;
        float acc = 0.f;
        for (int round = 0; round < k; ++round) {
            float h = c[0];
#pragma unroll
            for (int u = 1; u < kCandMean / 64; ++u) h = fmaxf(h, c[u]);
            float m = h;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
            const unsigned long long bal = __ballot(h == m);
            if (lane == __ffsll((long long)bal) - 1) {       // remove ONE instance of the maximum
                bool done = false;
#pragma unroll
                for (int u = 0; u < kCandMean / 64; ++u)
                    if (!done && c[u] == m) { c[u] = -INFINITY; done = true; }
            }
            acc += m;
        }
        result = acc / (float)k;
    }
    if (lane == 0) out[out_index ? out_index[row] : row] = result;
}

__global__ void csls_apply_kernel(float *__restrict__ s, int64_t n1, int64_t n2, int64_t ld,
                                  const float *__restrict__ r, const float *__restrict__ c) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = blockIdx.y;
    if (j < n2) s[i * ld + j] = (2.0f * s[i * ld + j] - r[i]) - c[j];
}

// ---- CSLS means in ONE sweep (similarity.py:57-83 without S or S^T in HBM) ------------------------------------------------
// r_i = mean of the k largest of row i of S = e1 e2^T, c_j = the same for column j.  Both are top-k problems with k ~ 10, so
// a per-row / per-column threshold estimated from a strided sample (as in the strip-free neighbour search, topk.hip) lets
// the tile sweep keep the few hundred values that can matter: the query side in lane-private list segments (no atomics),
// the candidate side in one list per candidate (a returning atomic per survivor: ~1 % of the values).  The exact top-k
// means come from the lists, summed in DESCENDING order like row_topk_mean_kernel (bit-identical with oracle_topk_mean).
// Rows / columns whose list overflowed or fell short are redone from a recomputed strip (bulk: <= 128 of each).
// BF16 (round 4): q / c are the hi / lo split rows, the values v~ are within *tol_ptr of the exact ones, both cuts are lowered
// by that bound and every list entry is a PAIR (v~, index of the other side) -- list_mean_rows_kernel<true> finds the entries that
// can belong to the exact top k and recomputes them with the exact chain.
// NW = 8 (BF16, K > 128): 512 threads on 256-candidate tiles through the three-stage ring (tile_pipeline_bf16_big, dynamic LDS);
// the query lists then have 8 * chunks segments (one per chunk, wave row and half-wave)
template <bool BF16, int NCH = 0, int NW = 4>
__global__ __launch_bounds__(NW * 64, 2) void csls_append_kernel(
    const float *__restrict__ q, int64_t nq, int ldq, const float *__restrict__ c, int64_t nc, int ldc, int dim,
    const float *__restrict__ thr_q, const float *__restrict__ thr_c, int tiles_per_chunk, int cap, int ccap,
    float *__restrict__ qlists, int32_t *__restrict__ qcounts, float *__restrict__ clists, int32_t *__restrict__ ccounts,
    const float *__restrict__ tol_ptr, TileGrid tg) {
    constexpr uint32_t ES = BF16 ? 8u : 4u;                 // bytes per list entry
    constexpr int MT = NW * 32;                             // candidate rows of a tile
    extern __shared__ __attribute__((aligned(16))) float csls_dyn_lds[];          // NW == 8: BIG_LDS_BYTES
    __shared__ __attribute__((aligned(16))) float lds_static[NW == 8 ? 4 : (NCH > 0 ? 4 * TILE * PLD : 4 * TILE * LDS_LD)];
    float *lds = NW == 8 ? csls_dyn_lds : lds_static;
    float *As = lds, *Bs = lds + 2 * TILE * LDS_LD;
    unsigned bx, by;
    if (!tile_grid_item(tg, bx, by)) return;
    // candidate j owns 2 * nqt segments of ccap values: one per (query tile, wave column) -- written by ONE wave, whose
    // half-waves hold the same candidate for 32 queries each: slots = prefix counts of a wave ballot (no atomics, no barrier;
    // the first version took a returning LDS atomic per survivor between two barriers per tile)
    const int nqt = (int)tg.nx, qt = (int)bx;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int half = lane >> 5, l32 = lane & 31;
    const int64_t q0 = (int64_t)bx * TILE;
    const int64_t nct = (nc + MT - 1) / MT;
    const int64_t ct_begin = (int64_t)by * tiles_per_chunk;
    const int64_t ct_end = (ct_begin + tiles_per_chunk < nct) ? ct_begin + tiles_per_chunk : nct;
    const int nseg = NW * (int)tg.ny;
    const int sidx = ((int)by * (NW / 2) + wm) * 2 + half;
    float th[2];
    uint32_t boff[2], bbeg[2], blast[2];
    int64_t qi[2];
    const float tol = BF16 ? *tol_ptr : 0.f;
    char *__restrict__ vbase = reinterpret_cast<char *>(qlists) + (size_t)q0 * nseg * cap * ES;
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
        const int ql = wn * 64 + tn * 32 + l32;
        qi[tn] = q0 + ql;
        th[tn] = qi[tn] < nq ? thr_q[qi[tn]] - tol : INFINITY;
        bbeg[tn] = boff[tn] = ES * (uint32_t)((ql * nseg + sidx) * cap);
        blast[tn] = boff[tn] + ES * (uint32_t)(cap - 1);
    }
    const int jl0 = wm * 64 + 4 * half;
    const int my_jl = jl0 + (l32 >> 4) * 32 + (l32 & 3) + 8 * ((l32 & 15) >> 2);     // lane l32 = tm * 16 + r looks after that candidate
    const uint32_t below = (1u << l32) - 1u;
    auto epilogue = [&](int64_t t, f32x16 (&acc)[2][2]) {
            const int64_t c0 = (ct_begin + t) * MT;
            const int64_t my_j = c0 + my_jl;
            const float my_tc = my_j < nc ? thr_c[my_j] - tol : INFINITY;
            int my_cnt = 0;
            // k ~ 10: ~0.05 % of the values survive either threshold, so most accumulator registers hold none.  One bound per
            // lane -- the smaller of its own query thresholds and the smallest candidate threshold of this tile's wave --
            // lets a register be skipped with two compares and a ballot instead of the slot arithmetic below (which cost the
            // means sweep 12.3 ms against 9.5 ms for the plain rank sweep at 70,000^2)
            float tc_min = my_tc;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) tc_min = fminf(tc_min, __shfl_xor(tc_min, off, 64));
            const float lo0 = fminf(th[0], tc_min), lo1 = fminf(th[1], tc_min);
#pragma unroll
            for (int tm = 0; tm < 2; ++tm) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if (__ballot(acc[tm][0][r] >= lo0 || acc[tm][1][r] >= lo1) == 0ull) continue;
                    const int jl = jl0 + tm * 32 + (r & 3) + 8 * (r >> 2);
                    const int j = (int)c0 + jl;
                    const bool jin = j < nc;
                    const float tc = __shfl(my_tc, (lane & 32) + tm * 16 + r, 64);
                    char *__restrict__ seg = reinterpret_cast<char *>(clists) + (size_t)((((int64_t)j * nqt + qt) * 2 + wn) * ccap) * ES;
                    int cnt = 0;
#pragma unroll
                    for (int tn = 0; tn < 2; ++tn) {
                        const float v = acc[tm][tn][r];
                        if (v >= th[tn] && jin) {
                            if constexpr (BF16) *reinterpret_cast<uint2 *>(vbase + min(boff[tn], blast[tn])) = make_uint2(__float_as_uint(v), (uint32_t)j);
                            else *reinterpret_cast<float *>(vbase + min(boff[tn], blast[tn])) = v;
                            boff[tn] += ES;
                        }
                        const bool pc = v >= tc && qi[tn] < nq;      // tc = +inf past the last candidate
                        const unsigned long long bal = __ballot(pc);
                        const uint32_t bh = half ? (uint32_t)(bal >> 32) : (uint32_t)bal;
                        const int slot = cnt + __popc(bh & below);
                        if (pc && slot < ccap) {
                            if constexpr (BF16) reinterpret_cast<uint2 *>(seg)[slot] = make_uint2(__float_as_uint(v), (uint32_t)qi[tn]);
                            else reinterpret_cast<float *>(seg)[slot] = v;
                        }
                        cnt += __popc(bh);
                    }
                    if (l32 == tm * 16 + r) my_cnt = cnt;
                }
            }
            if (my_j < nc) ccounts[(my_j * nqt + qt) * 2 + wn] = my_cnt;
        };
    auto m_tile = [=](int64_t t) { return (ct_begin + t) * MT; };
    const int64_t n_tiles = ct_end > ct_begin ? ct_end - ct_begin : 0;
    if constexpr (BF16 && NW == 8) tile_pipeline_bf16_big<true>(c, ldc, q, dim, q0, n_tiles, m_tile, lds, epilogue);
    else if constexpr (BF16 && NCH > 0) tile_pipeline_bf16_breg<NCH>(c, ldc, q, q0, n_tiles, m_tile, As, epilogue, dim);
    else if constexpr (BF16) tile_pipeline_bf16<true>(c, ldc, q, dim, q0, n_tiles, m_tile, As, Bs, epilogue);
    else tile_pipeline_packed(c, ldc, q, dim, q0, n_tiles, m_tile, As, Bs, epilogue);
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
        if (qi[tn] < nq) qcounts[qi[tn] * nseg + sidx] = (int32_t)((boff[tn] - bbeg[tn]) / ES);
}

constexpr int kMeanRegs = 16;                 // list values per lane: lists of up to 1,024 survivors
constexpr int kMeanSeg = 2048;               // segments per list (rows: 4 * chunks; columns: two per query tile)

// mean of the k largest of `cnt` values held kMeanRegs per lane (-inf padded): k rounds of wave-wide maximum, summed in
// descending order -- the arithmetic of row_topk_mean_kernel
__device__ __forceinline__ float wave_topk_mean(float (&c)[kMeanRegs], int k, int lane) {
    float acc = 0.f;
    for (int round = 0; round < k; ++round) {
        float h = c[0];
#pragma unroll
        for (int u = 1; u < kMeanRegs; ++u) h = fmaxf(h, c[u]);
        float m = h;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
        const unsigned long long bal = __ballot(h == m);
        if (lane == __ffsll((long long)bal) - 1) {       // remove ONE instance of the maximum
            bool done = false;
#pragma unroll
            for (int u = 0; u < kMeanRegs; ++u)
                if (!done && c[u] == m) { c[u] = -INFINITY; done = true; }
        }
        acc += m;
    }
    return acc / (float)k;
}

// one wave per query row: its survivors sit in nseg segments of `cap`
// BF16: the entries are pairs (v~, index); with t~ = the k-th largest v~ every entry that can belong to the exact top k has
// v~ >= t~ - 2 tol (|t - t~| <= tol for the exact k-th value t); those -- k plus a few, at most 64 -- are recomputed with the exact
// k-ordered chain (row `row` of a against row `index` of b), and the mean is the sum of the k largest of THEM in descending
// order: row_topk_mean_kernel's arithmetic on row_topk_mean_kernel's values.  The band has to lie inside the list
// (t~ - 2 tol >= thr - tol, the sweep's cut); otherwise the row fails over to the strip fallback like an overflowed one.
template <bool BF16>
__global__ __launch_bounds__(256) void list_mean_rows_kernel(const float *__restrict__ lists, const int32_t *__restrict__ counts,
                                                             int nseg, int cap, int64_t n_rows, int k, float *__restrict__ out,
                                                             int32_t *__restrict__ fail_rows, int32_t *__restrict__ n_fail,
                                                             const float *__restrict__ a, int lda, const float *__restrict__ b, int ldb,
                                                             int dim, const float *__restrict__ thr, const float *__restrict__ tol_ptr) {
    __shared__ int s_off[4][kMeanSeg + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * 4 + wave;
    if (row >= n_rows) return;
    int *off = s_off[wave];
    bool bad = false;
    for (int sg = lane; sg < nseg; sg += 64) {
        const int c = counts[row * nseg + sg];
        off[sg + 1] = c;
        bad |= c > cap;
    }
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
    {   // lengths -> offsets: every lane scans a contiguous run of segments, the runs are chained by a wave scan
        const int per = (nseg + 63) >> 6;
        int mine = 0;
        for (int u = 0; u < per; ++u) {
            const int sg = lane * per + u;
            if (sg < nseg) mine += off[sg + 1];
        }
        int incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        int run = incl - mine;
        for (int u = 0; u < per; ++u) {
            const int sg = lane * per + u;
            if (sg < nseg) { run += off[sg + 1]; off[sg + 1] = run; }
        }
        if (lane == 0) off[0] = 0;
    }
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
    const int total = off[nseg];
    bad = __ballot(bad) != 0ull || total < k || total > kMeanRegs * 64;
    if (bad) {
        if (lane == 0) fail_rows[atomicAdd(n_fail, 1)] = (int32_t)row;
        return;
    }
    float c[kMeanRegs];
    uint32_t id[BF16 ? kMeanRegs : 1];
    const float *base = lists + row * nseg * (int64_t)cap * (BF16 ? 2 : 1);
#pragma unroll
    for (int u = 0; u < kMeanRegs; ++u) {
        const int i = u * 64 + lane;
        c[u] = -INFINITY;
        if (BF16) id[u] = 0u;
        if (i < total) {
            int lo = 0, hi = nseg;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (off[mid] <= i) lo = mid; else hi = mid;
            }
            if constexpr (BF16) {
                const uint2 pr = reinterpret_cast<const uint2 *>(base)[(int64_t)lo * cap + (i - off[lo])];
                c[u] = __uint_as_float(pr.x);
                id[u] = pr.y;
            } else {
                c[u] = base[(int64_t)lo * cap + (i - off[lo])];
            }
        }
    }
    if constexpr (!BF16) {
        const float res = wave_topk_mean(c, k, lane);
        if (lane == 0) out[row] = res;
    } else {
        const float tol = *tol_ptr;
        float tk = INFINITY;                                   // t~: the k-th largest approximate value (k rounds of wave maximum)
        {
            float cc[kMeanRegs];
#pragma unroll
            for (int u = 0; u < kMeanRegs; ++u) cc[u] = c[u];
            for (int round = 0; round < k; ++round) {
                float h = cc[0];
#pragma unroll
                for (int u = 1; u < kMeanRegs; ++u) h = fmaxf(h, cc[u]);
                float m = h;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
                const unsigned long long bal = __ballot(h == m);
                if (lane == __ffsll((long long)bal) - 1) {
                    bool done = false;
#pragma unroll
                    for (int u = 0; u < kMeanRegs; ++u)
                        if (!done && cc[u] == m) { cc[u] = -INFINITY; done = true; }
                }
                tk = m;
            }
        }
        const float lo2 = tk - 2.0f * tol;
        int *cand = off;                                        // the offsets are dead: 64 candidate indices per wave
        int ncand = 0;
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int u = 0; u < kMeanRegs; ++u) {
            const bool in = c[u] >= lo2;
            const unsigned long long bal = __ballot(in);
            const int at = ncand + __popcll(bal & ((1ull << lane) - 1ull));
            if (in && at < 64) cand[at] = (int)id[u];
            ncand += __popcll(bal);
        }
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        if (ncand > 64 || lo2 < thr[row] - tol) {
            if (lane == 0) fail_rows[atomicAdd(n_fail, 1)] = (int32_t)row;
            return;
        }
        float e = -INFINITY;
        if (lane < ncand) {
            const float *__restrict__ x = a + row * lda, *__restrict__ y = b + (int64_t)cand[lane] * ldb;
            float acc = 0.f;
            int kk = 0;
            for (; kk + 32 <= dim; kk += 32) {                      // 16 loads in flight, then the chain in k order
                float4 xv[8], yv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) { xv[u] = oea::ld4(x + kk + 4 * u); yv[u] = oea::ld4(y + kk + 4 * u); }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    acc = fmaf(xv[u].x, yv[u].x, acc); acc = fmaf(xv[u].y, yv[u].y, acc);
                    acc = fmaf(xv[u].z, yv[u].z, acc); acc = fmaf(xv[u].w, yv[u].w, acc);
                }
            }
            for (; kk + 4 <= dim; kk += 4) {
                const float4 xv = oea::ld4(x + kk), yv = oea::ld4(y + kk);
                acc = fmaf(xv.x, yv.x, acc); acc = fmaf(xv.y, yv.y, acc); acc = fmaf(xv.z, yv.z, acc); acc = fmaf(xv.w, yv.w, acc);
            }
            for (; kk < dim; ++kk) acc = fmaf(x[kk], y[kk], acc);
            e = acc;
        }
        float acc = 0.f;
        for (int round = 0; round < k; ++round) {
            float m = e;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
            const unsigned long long bal = __ballot(e == m);
            if (lane == __ffsll((long long)bal) - 1) e = -INFINITY;
            acc += m;
        }
        if (lane == 0) out[row] = acc / (float)k;
    }
}

// failed rows beyond the bulk path (adversarial inputs): the row by the k-ordered fmaf chain into scratch, then the exact mean
__global__ __launch_bounds__(256) void slow_mean_rows_kernel(const float *__restrict__ a, int lda, const float *__restrict__ b, int64_t nb,
                                                             int ldb, int dim, int k, float *__restrict__ out,
                                                             const int32_t *__restrict__ fail_rows, const int32_t *__restrict__ n_fail,
                                                             int first, float *__restrict__ scratch, int64_t ld) {
    __shared__ float qs[2048];
    const int nf = *n_fail;
    float *srow = scratch + (int64_t)blockIdx.x * ld;
    for (int f = first + blockIdx.x; f < nf; f += gridDim.x) {
        const int64_t row = fail_rows[f];
        for (int i = threadIdx.x; i < dim; i += 256) qs[i] = a[row * lda + i];
        __syncthreads();
        for (int64_t j = threadIdx.x; j < nb; j += 256) {
            const float *br = b + j * ldb;
            float acc = 0.f;
            for (int kk = 0; kk < dim; ++kk) acc = fmaf(qs[kk], br[kk], acc);
            srow[j] = acc;
        }
        __threadfence_block();
        __syncthreads();
        if (threadIdx.x < 64) {
            const float res = k <= 16 ? topk_mean_by_insertion<16>(srow, nb, k, threadIdx.x) : topk_mean_by_insertion<32>(srow, nb, k, threadIdx.x);
            if (threadIdx.x == 0) out[row] = res;
        }
        __syncthreads();
    }
}

// workspace layout of oea_csls_means
struct CslsPlan {
    bool ok = false;
    int sample = 0, r1 = 0, r2 = 0, cap = 0, ccap = 0, chunks = 0, nseg = 0, tpc = 0, nqt = 0;
    int64_t ld1 = 0, ld2 = 0;
    size_t off_thr1, off_thr2, off_qcnt, off_ccnt, off_fail1, off_fail2, off_nfail, off_qlists, off_clists, off_strip, off_fbq,
        off_scratch, total;
};
constexpr int kCslsFb = 128, kCslsSlow = 64;

// big: the sweep runs on 256-candidate tiles with 8 waves (csls_append_kernel<.., 8>): chunks count those tiles, 8 segments per chunk
static CslsPlan plan_csls(int64_t n1, int64_t n2, int k, int big = 0 /* candidate rows of a big tile: 0 or 256 */) {
    CslsPlan p;
    if (n1 < 4096 || n2 < 4096 || k > 32) return p;
    p.sample = std::max(n1, n2) >= 32768 ? 4096 : 1024;       // keeps r n / S, the survivors per row, in the low hundreds
    static const int env_sample = [] { const char *e = getenv("OEA_CSLS_SAMPLE"); return e ? atoi(e) : 0; }();       // experiments
    if (env_sample == 1024 || env_sample == 2048 || env_sample == 4096) p.sample = env_sample;
    auto rank_of = [&](int64_t n) { const double e = (double)k * p.sample / (double)n; return (int)(e + 3.5 * std::sqrt(e) + 8.0); };
    p.r1 = rank_of(n2);                       // thresholds of the rows of S (queries against sampled candidates)
    p.r2 = rank_of(n1);
    const double m1 = (double)p.r1 * n2 / p.sample, m2 = (double)p.r2 * n1 / p.sample;      // survivors per row / per column
    if (m1 * (1.0 + 5.0 / std::sqrt((double)p.r1)) > kMeanRegs * 64 || m2 * (1.0 + 5.0 / std::sqrt((double)p.r2)) > kMeanRegs * 64) return p;
    p.chunks = pick_chunks(oea::ceil_div(n1, TILE), oea::ceil_div(n2, big ? big : TILE), &p.tpc);
    p.nseg = (big ? big / 32 : 4) * p.chunks;
    if (p.nseg > kMeanSeg) return p;
    // the threshold is the r-th of a sample: the survivor count of a row scales with a factor of relative spread 1 / sqrt(r)
    // COMMON to its segments, on top of each segment's own sqrt(m) noise
    p.nqt = (int)oea::ceil_div(n1, TILE);
    if (2 * p.nqt > kMeanSeg) return p;
    const double ms = m1 / p.nseg, mc = m2 / (2 * p.nqt);        // column lists: one segment per (query tile, wave column)
    p.cap = ((int)(ms * (1.0 + 5.0 / std::sqrt((double)p.r1)) + 8.0 * std::sqrt(ms) + 16.0) + 7) / 8 * 8;
    p.ccap = ((int)(mc * (1.0 + 5.0 / std::sqrt((double)p.r2)) + 8.0 * std::sqrt(mc) + 8.0) + 3) / 4 * 4;
    if ((size_t)128 * p.nseg * p.cap * 8 >= ((size_t)1 << 32)) return p;
    p.ld1 = (n1 + 31) / 32 * 32;
    p.ld2 = (n2 + 31) / 32 * 32;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
    p.off_thr1 = take(4 * (size_t)n1); p.off_thr2 = take(4 * (size_t)n2);
    p.off_qcnt = take(4 * (size_t)n1 * p.nseg); p.off_ccnt = take(4 * (size_t)n2 * 2 * p.nqt);
    p.off_fail1 = take(4 * (size_t)n1); p.off_fail2 = take(4 * (size_t)n2); p.off_nfail = take(256);
    p.off_qlists = take(8 * (size_t)n1 * p.nseg * p.cap);             // 8 B per entry: (value, index) pairs under the bf16 sweep
    p.off_clists = take(8 * (size_t)n2 * 2 * p.nqt * p.ccap);
    // sample strips; the fallback strip [kCslsFb, max ld] reuses the space after the thresholds are taken
    p.off_strip = take(4 * std::max<size_t>((size_t)std::max(n1, n2) * p.sample, (size_t)kCslsFb * std::max(p.ld1, p.ld2)));
    p.off_fbq = take(4 * (size_t)kCslsFb * 4096);
    p.off_scratch = take(4 * (size_t)kCslsSlow * std::max(p.ld1, p.ld2));
    p.total = off;
    p.ok = true;
    return p;
}

}  // namespace

extern "C" {

int oea_row_topk_mean(const float *s, int64_t n1, int64_t n2, int64_t ld, int32_t k, float *out, void *stream) {
    OEA_REQUIRE(s && out, "null pointer");
    OEA_REQUIRE(k >= 1 && k <= 32 && k <= n2, "1 <= k <= min(32, n2)");
    if (n1 == 0) return OEA_OK;
    hipStream_t st = oea::as_stream(stream);
    const unsigned grid = (unsigned)oea::ceil_div(n1, 4);
    row_topk_mean_kernel<<<grid, 256, 0, st>>>(s, n1, n2, ld, k, out, nullptr, nullptr);
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

size_t oea_csls_means_workspace_bytes(int64_t n1, int64_t n2, int32_t k) {
    const CslsPlan p = plan_csls(n1, n2, k), pb = plan_csls(n1, n2, k, BIG_MT);   // (the call picks one by the row width)
    return p.ok ? std::max(p.total, pb.ok ? pb.total : 0) : 0;
}

int oea_csls_means(const float *e1, int64_t n1, int32_t ld1, const float *e2, int64_t n2, int32_t ld2, int32_t dim, int32_t k,
                   float *r_out, float *c_out, void *workspace, size_t ws_bytes, void *stream) {
    OEA_REQUIRE(e1 && e2 && r_out && c_out && workspace, "null pointer");
    OEA_REQUIRE(ld1 % 4 == 0 && ld2 % 4 == 0 && dim > 0 && dim <= ld1 && dim <= ld2 && dim <= 2048, "ld % 4 == 0, dim <= min(ld, 2048)");
    OEA_REQUIRE(k >= 1 && k <= n1 && k <= n2, "1 <= k <= min(n1, n2)");
    // from 3e8 pairs on the sweep multiplies the bf16 hi / lo split (3/16 of the fp32 matrix time, see the prefilter section);
    // the means are still those of the exact values (list_mean_rows_kernel<true>).  OEA_CSLS_BF16=0 keeps the fp32 sweep.
    // (both read per call: the tests move the limit).  Rows wider than 128: 256-candidate tiles, 512 threads, three-stage ring.
    const char *env_on = getenv("OEA_CSLS_BF16"), *env_min = getenv("OEA_CSLS_BF16_MIN_PAIRS");
    const bool bf16_on = !(env_on && env_on[0] == '0');
    const double bf16_min = env_min ? atof(env_min) : 3e8;
    const bool bf16 = bf16_on && (double)n1 * (double)n2 >= bf16_min;
    static const bool big_on = [] { const char *e = getenv("OEA_BF16_BIG"); return !(e && e[0] == '0'); }();
    const bool big = bf16 && big_on && (dim + BK - 1) / BK * BK > 128 && plan_csls(n1, n2, k, BIG_MT).ok;
    const CslsPlan p = plan_csls(n1, n2, k, big ? BIG_MT : 0);
    if (!p.ok) { oea::set_error("oea_csls_means: shape not covered (n1, n2 >= 4096, k <= 32)"); return OEA_EUNSUPPORTED; }
    OEA_REQUIRE(ws_bytes >= p.total, "workspace smaller than oea_csls_means_workspace_bytes");
    hipStream_t st = oea::as_stream(stream);
    char *w = static_cast<char *>(workspace);
    float *thr1 = reinterpret_cast<float *>(w + p.off_thr1), *thr2 = reinterpret_cast<float *>(w + p.off_thr2);
    int32_t *qcnt = reinterpret_cast<int32_t *>(w + p.off_qcnt), *ccnt = reinterpret_cast<int32_t *>(w + p.off_ccnt);
    int32_t *fail1 = reinterpret_cast<int32_t *>(w + p.off_fail1), *fail2 = reinterpret_cast<int32_t *>(w + p.off_fail2);
    int32_t *nfail = reinterpret_cast<int32_t *>(w + p.off_nfail);          // [0] rows, [1] columns
    float *qlists = reinterpret_cast<float *>(w + p.off_qlists), *clists = reinterpret_cast<float *>(w + p.off_clists);
    float *strip = reinterpret_cast<float *>(w + p.off_strip), *fbq = reinterpret_cast<float *>(w + p.off_fbq);
    float *scratch = reinterpret_cast<float *>(w + p.off_scratch);
    PackedOp p1, p2, s1, s2, b1, b2;
    int rc = pack_operand(0, e1, n1, ld1, dim, st, &p1);          // (fp32 packs: the exact strips of the fallbacks)
    if (rc == OEA_OK) rc = pack_operand(1, e2, n2, ld2, dim, st, &p2);
    if (rc != OEA_OK) return rc;
    const int kp = p1.kp;
    OEA_REQUIRE(kp <= 4096, "dim <= 4096");
    // thresholds: rows of S against sampled candidates (every (n2 / S)-th), columns against sampled queries.  Under the bf16 sweep
    // the sample strips are bf16 products too (round 5): a threshold is an ESTIMATE of where the k-th value lies -- the lists are
    // cut below it by the bound and rows whose list comes out short or long take the exact fallback either way -- and at K = 1,200
    // the two fp32 strips cost 10.9 ms of a 90 ms evaluation
    static const bool bf16_strips = [] { const char *e = getenv("OEA_CSLS_BF16_STRIPS"); return !(e && e[0] == '0'); }();
    if (bf16) {
        rc = pack_operand_bf16(4, e1, n1, ld1, dim, st, &b1);
        if (rc == OEA_OK) rc = pack_operand_bf16(5, e2, n2, ld2, dim, st, &b2);
        if (rc != OEA_OK) return rc;
    }
    if (bf16 && bf16_strips) {
        rc = pack_operand_bf16(2, e2, p.sample, ld2 * (int)(n2 / p.sample), dim, st, &s2);
        if (rc == OEA_OK) rc = pack_operand_bf16(3, e1, p.sample, ld1 * (int)(n1 / p.sample), dim, st, &s1);
        if (rc != OEA_OK) return rc;
        sample_strip_bf16_launch(b1.p, n1, s2.p, p.sample, kp, dim, strip, st);
        rc = oea::kth_value(strip, n1, p.sample, p.r1, thr1, st);
        if (rc != OEA_OK) return rc;
        sample_strip_bf16_launch(b2.p, n2, s1.p, p.sample, kp, dim, strip, st);
        rc = oea::kth_value(strip, n2, p.sample, p.r2, thr2, st);
        if (rc != OEA_OK) return rc;
    } else {
        rc = pack_operand(2, e2, p.sample, ld2 * (int)(n2 / p.sample), dim, st, &s2);
        if (rc == OEA_OK) rc = pack_operand(3, e1, p.sample, ld1 * (int)(n1 / p.sample), dim, st, &s1);
        if (rc != OEA_OK) return rc;
        sim_inner_store_packed(p1.p, n1, s2.p, p.sample, kp, dim, strip, p.sample, st);
        rc = oea::kth_value(strip, n1, p.sample, p.r1, thr1, st);
        if (rc != OEA_OK) return rc;
        sim_inner_store_packed(p2.p, n2, s1.p, p.sample, kp, dim, strip, p.sample, st);
        rc = oea::kth_value(strip, n2, p.sample, p.r2, thr2, st);
        if (rc != OEA_OK) return rc;
    }
    // every (candidate, query tile) count is written by the sweep when chunks cover all candidate tiles -- they do
    OEA_CHECK_HIP(hipMemsetAsync(nfail, 0, 256, st));
    const TileGrid grid = make_tile_grid((unsigned)oea::ceil_div(n1, TILE), (unsigned)p.chunks);
    if (bf16) {
        float *tol = reinterpret_cast<float *>(nfail + 16);                // [0] the bound, [1] / [2] max row norms (zeroed above)
        bf16_tol_bound(e1, n1, ld1, e2, n2, ld2, dim, true, tol, st);
        static const bool breg_on = [] { const char *e = getenv("OEA_BF16_BREG"); return !(e && e[0] == '0'); }();
#define OEA_CSLS_APPEND(N) csls_append_kernel<true, N><<<tile_grid_blocks(grid), 256, 0, st>>>(b1.p, n1, kp, b2.p, n2, kp, dim, thr1, thr2, p.tpc, \
                                                                                                   p.cap, p.ccap, qlists, qcnt, clists, ccnt, tol, grid)
        if (big) {
            OEA_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(csls_append_kernel<true, 0, 8>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, BIG_LDS_BYTES));   // per device
            csls_append_kernel<true, 0, 8><<<tile_grid_blocks(grid), 512, BIG_LDS_BYTES, st>>>(
                b1.p, n1, kp, b2.p, n2, kp, dim, thr1, thr2, p.tpc, p.cap, p.ccap, qlists, qcnt, clists, ccnt, tol, grid);
            OEA_CHECK_HIP(hipGetLastError());
        } else switch ((breg_on && kp <= 128) ? kp / 32 : 0) {
            case 4: OEA_CSLS_APPEND(4); break;
            case 3: OEA_CSLS_APPEND(3); break;
            case 2: OEA_CSLS_APPEND(2); break;
            case 1: OEA_CSLS_APPEND(1); break;
            default: OEA_CSLS_APPEND(0); break;
        }
#undef OEA_CSLS_APPEND
        list_mean_rows_kernel<true><<<(unsigned)oea::ceil_div(n1, 4), 256, 0, st>>>(qlists, qcnt, p.nseg, p.cap, n1, k, r_out, fail1, nfail,
                                                                                    e1, ld1, e2, ld2, dim, thr1, tol);
        list_mean_rows_kernel<true><<<(unsigned)oea::ceil_div(n2, 4), 256, 0, st>>>(clists, ccnt, 2 * p.nqt, p.ccap, n2, k, c_out, fail2,
                                                                                    nfail + 1, e2, ld2, e1, ld1, dim, thr2, tol);
    } else {
        csls_append_kernel<false><<<tile_grid_blocks(grid), 256, 0, st>>>(p1.p, n1, kp, p2.p, n2, kp, dim, thr1, thr2, p.tpc, p.cap, p.ccap,
                                                                                 qlists, qcnt, clists, ccnt, nullptr, grid);
        list_mean_rows_kernel<false><<<(unsigned)oea::ceil_div(n1, 4), 256, 0, st>>>(qlists, qcnt, p.nseg, p.cap, n1, k, r_out, fail1, nfail,
                                                                                     nullptr, 0, nullptr, 0, 0, nullptr, nullptr);
        list_mean_rows_kernel<false><<<(unsigned)oea::ceil_div(n2, 4), 256, 0, st>>>(clists, ccnt, 2 * p.nqt, p.ccap, n2, k, c_out, fail2,
                                                                                     nfail + 1, nullptr, 0, nullptr, 0, 0, nullptr, nullptr);
    }
    // fallbacks (normally empty): bulk for the first kCslsFb failed rows / columns, slow kernel for the rest
    oea::gather_packed_rows(p1.p, kp, fail1, nfail, fbq, st);
    sim_inner_store_packed(fbq, kCslsFb, p2.p, n2, kp, dim, strip, p.ld2, st, nfail);
    row_topk_mean_kernel<<<kCslsFb / 4, 256, 0, st>>>(strip, kCslsFb, n2, p.ld2, k, r_out, fail1, nfail);
    slow_mean_rows_kernel<<<kCslsSlow, 256, 0, st>>>(e1, ld1, e2, n2, ld2, dim, k, r_out, fail1, nfail, kCslsFb, scratch, p.ld2);
    oea::gather_packed_rows(p2.p, kp, fail2, nfail + 1, fbq, st);
    sim_inner_store_packed(fbq, kCslsFb, p1.p, n1, kp, dim, strip, p.ld1, st, nfail + 1);
    row_topk_mean_kernel<<<kCslsFb / 4, 256, 0, st>>>(strip, kCslsFb, n1, p.ld1, k, c_out, fail2, nfail + 1);
    slow_mean_rows_kernel<<<kCslsSlow, 256, 0, st>>>(e2, ld2, e1, n1, ld1, dim, k, c_out, fail2, nfail + 1, kCslsFb, scratch, p.ld1);
    rc = release_packed(st);
    if (rc != OEA_OK) return rc;
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

int oea_csls_apply(float *s, int64_t n1, int64_t n2, int64_t ld, const float *r, const float *c, void *stream) {
    OEA_REQUIRE(s && r && c, "null pointer");
    if (n1 == 0 || n2 == 0) return OEA_OK;
    OEA_REQUIRE(n1 <= 65535 * 1024ll, "n1 too large for one launch");
    // grid.y is limited to 65535: loop over row blocks
    for (int64_t i0 = 0; i0 < n1; i0 += 65535) {
        const int64_t rows = std::min<int64_t>(65535, n1 - i0);
        csls_apply_kernel<<<dim3((unsigned)oea::ceil_div(n2, 256), (unsigned)rows), 256, 0, oea::as_stream(stream)>>>(
            s + i0 * ld, rows, n2, ld, r + i0, c);
    }
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

}  // extern "C"
