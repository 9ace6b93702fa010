// sim_rank.hip -- similarity tiles on the fp32 matrix cores + fused alignment-rank epilogue.
//
// Replaces sim() / csls_sim() / calculate_rank() of the reference's greedy_alignment
// (modules/finding/similarity.py:11-83, modules/finding/alignment.py:13-84,146-168):
//   np.matmul(e1, e2.T)             -> 128x128 tiles of v_mfma_f32_32x32x2_f32 (exact fp32:
//                                      a k-ordered fmaf chain, k = 0,1,2,... -- identical to
//                                      oracle/c/oracle.c:dot_chain, hence bit-exact ranks)
//   argsort(-row) + np.where(==gold) -> rank_i = #{j : S_ij > S_ii} (+ stable tie rule),
//                                      counted in the epilogue; the N1 x N2 matrix is never
//                                      written (19.6 GB at 70,000^2 in the reference)
//   scipy cdist('cityblock')         -> fp64 VALU tiles, sequential k (bit-exact vs scipy)
//
// Operand layout: the callers' tables are row-major [n, ld] fp32 (K contiguous).  Each call first
// packs both operands ([n_pad, Kp], the k index permuted inside groups of 8: positions 0..3 hold
// k = 0,2,4,6, 4..7 hold k = 1,3,5,7) so that one ds_read_b128 gives a lane its operand for four
// consecutive MFMA k-steps in natural k order; K-chunks of 32 then go HBM/L2 -> LDS by LDS-DMA
// (see "packed operands + LDS-DMA staging" in sim_tiles.h, which holds the tile pipelines).
//
// This file holds: the pack kernels and the process-wide operand slots, the strip store kernels, the fp32 and fp64 rank sweeps,
// the certified bf16 prefilter, and the oea_rank_* / oea_sim_* entry points.  It is also where everything sim_tiles.h declares
// for the other similarity files (topk.hip, csls_means.hip) is defined once.
#include "sim_tiles.h"
#include <stdlib.h>
#include <cmath>

using namespace oea;

namespace {

// fp32 operands: [n_pad, Kp], zero filled, every group of 8 k stored as k = 0,2,4,6,1,3,5,7 (see stage_packed, sim_tiles.h)

__global__ void pack_rows_kernel(const float *__restrict__ src, int64_t n, int ld, int dim, float *__restrict__ dst,
                                 int64_t n_pad, int kp) {
    const int cpr = kp / 4;                                            // 16-byte columns per packed row
    const int64_t total = n_pad * cpr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / cpr;
        const int c = (int)(i - row * cpr);
        const int k = 8 * (c >> 1) + (c & 1);                          // k, k+2, k+4, k+6
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < n) {
            const float *r = src + row * ld;
            if (k < dim) v.x = r[k];
            if (k + 2 < dim) v.y = r[k + 2];
            if (k + 4 < dim) v.z = r[k + 4];
            if (k + 6 < dim) v.w = r[k + 6];
        }
        oea::st4(dst + row * kp + 4 * c, v);
    }
}

// packed row = kp "float slots" (kp = dim rounded up to 32): every 32-k chunk is 128 B = 8 granules of 8 bf16; granule
// (s * 2 + h) * 2 + p holds k = 32 chunk + 16 s + 8 h + [0, 8) of the hi (p = 0) or lo (p = 1) part -- one MFMA operand of lane
// half h in k-step s.  Same bytes per row as the fp32 packed layout, so stage_packed moves it unchanged.
__global__ void pack_rows_bf16_kernel(const float *__restrict__ src, int64_t n, int ld, int dim, uint4 *__restrict__ dst,
                                      int64_t n_pad, int kp) {
    const int cpr = kp / 4;
    const int64_t total = n_pad * cpr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / cpr;
        const int c = (int)(i - row * cpr);
        const int g = c & 7, k0 = 32 * (c >> 3) + 16 * (g >> 2) + 8 * ((g >> 1) & 1), lo = g & 1;
        uint32_t h[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const float x = (row < n && k0 + t < dim) ? src[row * ld + k0 + t] : 0.f;
            const uint32_t hi = bf16_rne(x);
            h[t] = lo ? bf16_rne(x - __uint_as_float(hi << 16)) : hi;
        }
        dst[i] = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
    }
}

// max row norm of a table as the bits of a non-negative float (integer order == float order)
__global__ void row_norm_max_kernel(const float *__restrict__ src, int64_t n, int ld, int dim, unsigned *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float nr = 0.f;
    if (i < n) {
        float ss = 0.f;
        for (int k = 0; k < dim; ++k) ss = fmaf(src[i * ld + k], src[i * ld + k], ss);
        nr = sqrtf(ss) * 1.0000005f;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nr = fmaxf(nr, __shfl_xor(nr, off, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(out, __float_as_uint(nr));
}

// ---- gold similarity: S_ii as the same k-ordered fmaf chain (one lane per query) ---------------
__global__ void gold_inner_kernel(const float *__restrict__ e1, int64_t n1, int ld1, const float *__restrict__ e2,
                                  int ld2, int dim, const float *__restrict__ csls_r,
                                  const float *__restrict__ csls_c, float *__restrict__ gold) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n1) return;
    const float *a = e1 + i * ld1, *b = e2 + i * ld2;
    float acc = 0.f;
    int k = 0;
    for (; k + 4 <= dim; k += 4) {                    // 16-byte loads (ld % 4 == 0), the chain itself stays k-ordered
        const float4 x = oea::ld4(a + k), y = oea::ld4(b + k);
        acc = fmaf(x.x, y.x, acc); acc = fmaf(x.y, y.y, acc); acc = fmaf(x.z, y.z, acc); acc = fmaf(x.w, y.w, acc);
    }
    for (; k < dim; ++k) acc = fmaf(a[k], b[k], acc);
    if (csls_r) acc = (2.0f * acc - csls_r[i]) - csls_c[i];
    gold[i] = acc;
}

// ---- fused evaluation: ONE prologue launch + the sweep (oea_rank_eval_metrics) -------------------------------------------------
// The 10,500^2 evaluation of BASELINE configs[1] is a 0.20 ms tile sweep; with its operands packed by two launches, the gold
// similarities by a third, two memsets, the argmax extraction and the metric reduction by two more, and a zero-fill of the
// result buffer, the call took 0.28 ms.  Prologue: both packs + golds + zeroing in one grid-stride
// kernel.  Epilogue: the sweep's workgroups take a ticket after their integer atomics; the last one reads the merged ranks /
// keys back (device-coherent loads), writes argmax and reduces Hits@k / sum(rank + 1) / sum 1 / (rank + 1) in a fixed order.
struct EvalTail {
    unsigned *done;            // NULL: plain oea_rank_eval (argmax / metrics by separate launches); else [1 + query tiles] tickets
    int32_t *argmax;
    long long *hits;           // [nk], then rank_sum at hits[nk]
    double *rr_sum;
    long long *tile_part;      // [query tiles][10]: Hits@k x 8, sum(rank + 1), bits of the tile's sum 1 / (rank + 1)
    int tk[8];
    int nk;
};

// Two levels, so that nobody walks all n1 rows alone (a first version let the globally last workgroup read every rank with
// device-coherent loads: 41 dependent round trips per thread at n1 = 10,500 -- slower than the launches it replaced):
//  (1) the last of the gridDim.y workgroups of a QUERY TILE finalises the tile's 128 rows -- one coherent load per thread --
//      and leaves the tile's partial sums (integers; the reciprocal ranks added in a fixed order);
//  (2) the last tile to do so adds the partials in tile order.
__device__ __forceinline__ void eval_tail(const EvalTail &t, const int32_t *rank, const unsigned long long *best_key, int64_t n1,
                                          long long *s_i, double *s_d, int *s_flag) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // Everything the tail reads was written by device-scope ATOMICS (rank: atomicAdd, keys: atomicMax, tile partials:
    // atomic stores), i.e. at the point of coherence already -- ordering them before the ticket only needs this wave's
    // outstanding memory operations to have completed (s_waitcnt), NOT a cache action.  A __threadfence() here costs every
    // workgroup an L2 write-back + invalidate: the operand panels its XCD neighbours share in L2 are thrown away 2,000 times
    // per sweep (measured: 0.283 -> 0.365 ms per 10,500^2 evaluation, gpurun_out r03e / r03f).
    // The wait is spelled out: a workgroup-scope release need not lower to s_waitcnt vmcnt(0) when the
    // workgroup's waves share one L2 anyway (no tgsplit), and this wave's no-return atomics go to other L2 channels than the
    // ticket -- they must have been acknowledged before thread 0 takes it.  s_waitcnt 0 = vmcnt(0) expcnt(0) lgkmcnt(0).
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    if (tid == 0) *s_flag = atomicAdd(t.done + 1 + blockIdx.x, 1u) == gridDim.y - 1u;
    __syncthreads();
    if (!*s_flag) return;
    long long h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    double rr = 0.0;
    const int64_t i = (int64_t)blockIdx.x * TILE + tid;
    if (tid < TILE && i < n1) {
        const int r = __hip_atomic_load(rank + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // other XCDs' atomics
        const unsigned long long key = __hip_atomic_load(best_key + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        t.argmax[i] = (int32_t)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull));
#pragma unroll
        for (int k = 0; k < 8; ++k) h[k] = (k < t.nk && r < t.tk[k]);
        h[8] = r + 1;
        rr = 1.0 / (double)(r + 1);
    }
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) h[k] += __shfl_xor(h[k], off, 64);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) rr += __shfl_xor(rr, off, 64);
    if (lane == 0) {                 // the tile buffers are free: every wave is past its last MFMA chunk (barriers above)
#pragma unroll
        for (int k = 0; k < 9; ++k) s_i[wave * 9 + k] = h[k];
        s_d[wave] = rr;
    }
    __syncthreads();
    if (tid < 10) {
        long long v = 0;
        if (tid < 9) { for (int w = 0; w < 4; ++w) v += s_i[w * 9 + tid]; }
        else { double d = 0.0; for (int w = 0; w < 4; ++w) d += s_d[w]; v = __double_as_longlong(d); }
        __hip_atomic_store(t.tile_part + (int64_t)blockIdx.x * 10 + tid, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    if (tid == 0) *s_flag = atomicAdd(t.done, 1u) == gridDim.x - 1u;
    __syncthreads();
    if (!*s_flag) return;
    long long g[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    double grr = 0.0;
    for (int q = tid; q < (int)gridDim.x; q += blockDim.x) {
#pragma unroll
        for (int k = 0; k < 9; ++k) g[k] += __hip_atomic_load(t.tile_part + (int64_t)q * 10 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        grr += __longlong_as_double(__hip_atomic_load(t.tile_part + (int64_t)q * 10 + 9, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) g[k] += __shfl_xor(g[k], off, 64);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) grr += __shfl_xor(grr, off, 64);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) s_i[wave * 9 + k] = g[k];
        s_d[wave] = grr;
    }
    __syncthreads();
    if (tid < 9) {
        long long v = 0;
        for (int w = 0; w < 4; ++w) v += s_i[w * 9 + tid];
        if (tid < t.nk) t.hits[tid] = v;
        else if (tid == 8) t.hits[t.nk] = v;
    } else if (tid == 9) {
        double v = 0.0;
        for (int w = 0; w < 4; ++w) v += s_d[w];
        *t.rr_sum = v;
    }
}

__global__ __launch_bounds__(256) void eval_prologue_kernel(const float *__restrict__ e1, int64_t n1, int ld1,
                                                            const float *__restrict__ e2, int64_t n2, int ld2, int dim,
                                                            float *__restrict__ p1, int64_t n1_pad, float *__restrict__ p2,
                                                            int64_t n2_pad, int kp, const float *__restrict__ csls_r,
                                                            const float *__restrict__ csls_c, int64_t gold_off,
                                                            float *__restrict__ gold, unsigned long long *__restrict__ keys,
                                                            int32_t *__restrict__ rank, unsigned *__restrict__ done, int n_done) {
    const int cpr = kp / 4;
    const int64_t t1 = n1_pad * cpr, t2 = n2_pad * cpr;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = gid; i < t1 + t2; i += stride) {                 // pack_rows_kernel for both operands
        const bool second = i >= t1;
        const int64_t ii = second ? i - t1 : i;
        const int64_t row = ii / cpr;
        const int c = (int)(ii - row * cpr);
        const int k = 8 * (c >> 1) + (c & 1);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < (second ? n2 : n1)) {
            const float *r = second ? e2 + row * ld2 : e1 + row * ld1;
            if (k < dim) v.x = r[k];
            if (k + 2 < dim) v.y = r[k + 2];
            if (k + 4 < dim) v.z = r[k + 4];
            if (k + 6 < dim) v.w = r[k + 6];
        }
        oea::st4((second ? p2 : p1) + row * kp + 4 * c, v);
    }
    for (int64_t i = gid; i < n1; i += stride) {                      // gold_inner_kernel + the two memsets
        const float *a = e1 + i * ld1, *b = e2 + (gold_off + i) * ld2;
        float acc = 0.f;
        int k = 0;
        for (; k + 4 <= dim; k += 4) {
            const float4 x = oea::ld4(a + k), y = oea::ld4(b + k);
            acc = fmaf(x.x, y.x, acc); acc = fmaf(x.y, y.y, acc); acc = fmaf(x.z, y.z, acc); acc = fmaf(x.w, y.w, acc);
        }
        for (; k < dim; ++k) acc = fmaf(a[k], b[k], acc);
        if (csls_r) acc = (2.0f * acc - csls_r[i]) - csls_c[gold_off + i];
        gold[i] = acc;
        keys[i] = 0ull;
        rank[i] = 0;
    }
    for (int64_t i = gid; i < n_done; i += stride) done[i] = 0u;
}

// ---- fused rank epilogue: M = candidates (e2 rows), N = queries (e1 rows) -----------------------
// grid.x = query tiles, grid.y = candidate chunks.  Per lane: one query (MFMA column) and 16
// candidates per MFMA tile, so the per-query reductions stay in registers across the whole
// candidate sweep; partial results are merged with integer atomics (order independent).
template <bool CSLS>
__global__ __launch_bounds__(256, 2) void rank_inner_kernel(
    const float *__restrict__ e1, int64_t n1, int ld1, const float *__restrict__ e2, int64_t n2, int ld2,
    int dim, const float *__restrict__ gold, const float *__restrict__ csls_r, const float *__restrict__ csls_c,
    int tiles_per_chunk, int64_t gold_off, int32_t *__restrict__ rank, unsigned long long *__restrict__ best_key,
    EvalTail tail) {
    __shared__ __attribute__((aligned(16))) float As[2 * TILE * LDS_LD];
    __shared__ __attribute__((aligned(16))) float Bs[2 * TILE * LDS_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int64_t q0 = (int64_t)blockIdx.x * TILE;
    const int64_t nct = (n2 + TILE - 1) / TILE;
    const int64_t ct_begin = (int64_t)blockIdx.y * tiles_per_chunk;
    const int64_t ct_end = (ct_begin + tiles_per_chunk < nct) ? ct_begin + tiles_per_chunk : nct;

    int64_t qi[2];
    float g[2], rq[2];
    int cnt[2] = {0, 0};
    float best[2] = {-INFINITY, -INFINITY};
    int bidx[2] = {0x7fffffff, 0x7fffffff};
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
        qi[tn] = q0 + wn * 64 + tn * 32 + (lane & 31);
        const bool ok = qi[tn] < n1;
        g[tn] = ok ? gold[qi[tn]] : 0.f;
        rq[tn] = (ok && CSLS) ? csls_r[qi[tn]] : 0.f;
    }
    tile_pipeline_packed(
        e2, ld2, e1, dim, q0, ct_end > ct_begin ? ct_end - ct_begin : 0,
        [=](int64_t t) { return (ct_begin + t) * TILE; }, As, Bs,
        [&](int64_t t, f32x16 (&acc)[2][2]) {
            const int64_t c0 = (ct_begin + t) * TILE;
            const int64_t g_lo = q0 + gold_off;              // the golds of this query tile: columns [g_lo, g_lo + 128)
            const int jb = (int)c0 + wm * 64 + 4 * (lane >> 5);
            const bool below = c0 + TILE <= g_lo, above = c0 >= g_lo + TILE;
            if (c0 + TILE <= n2 && (below || above)) {
                // interior tile away from the golds: every j is on one side of every gold, so the tie
                // rule is a plain >= (j < gold) or > (j > gold); a lane meets its candidates in
                // ascending j, so a strict > keeps the smallest argmax
#pragma unroll
                for (int tm = 0; tm < 2; ++tm) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int j = jb + tm * 32 + (r & 3) + 8 * (r >> 2);
                        const float cj = CSLS ? csls_c[j] : 0.f;
#pragma unroll
                        for (int tn = 0; tn < 2; ++tn) {
                            float v = acc[tm][tn][r];
                            if (CSLS) v = fmaf(2.0f, v, -rq[tn]) - cj;       // 2v is exact: == (2v - r) - c
                            cnt[tn] += below ? (v >= g[tn]) : (v > g[tn]);
                            if (v > best[tn]) { best[tn] = v; bidx[tn] = j; }
                        }
                    }
                }
                return;
            }
#pragma unroll
            for (int tm = 0; tm < 2; ++tm) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t j = jb + tm * 32 + (r & 3) + 8 * (r >> 2);
                    if (j < n2) {
                        const float cj = CSLS ? csls_c[j] : 0.f;
#pragma unroll
                        for (int tn = 0; tn < 2; ++tn) {
                            float v = acc[tm][tn][r];
                            if (CSLS) v = fmaf(2.0f, v, -rq[tn]) - cj;
                            const int64_t i = qi[tn];
                            cnt[tn] += (j != i + gold_off) && (v > g[tn] || (v == g[tn] && j < i + gold_off));
                            if (v > best[tn] || (v == best[tn] && (int)j < bidx[tn])) { best[tn] = v; bidx[tn] = (int)j; }
                        }
                    }
                }
            }
        });
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
        // merge the two half-waves (same query, disjoint candidates)
        cnt[tn] += __shfl_xor(cnt[tn], 32, 64);
        const float ob = __shfl_xor(best[tn], 32, 64);
        const int oi = __shfl_xor(bidx[tn], 32, 64);
        if (ob > best[tn] || (ob == best[tn] && oi < bidx[tn])) { best[tn] = ob; bidx[tn] = oi; }
        if (lane < 32 && qi[tn] < n1 && ct_end > ct_begin) {
            if (cnt[tn]) atomicAdd(rank + qi[tn], cnt[tn]);
            const unsigned long long key = ((unsigned long long)f2ord(best[tn]) << 32) | (0xFFFFFFFFu - (uint32_t)bidx[tn]);
            atomicMax(best_key + qi[tn], key);
        }
    }
    if (tail.done) {                 // fused evaluation (oea_rank_eval_metrics): the last workgroups to arrive finish the job
        __shared__ int s_flag;
        eval_tail(tail, rank, best_key, n1, reinterpret_cast<long long *>(As), reinterpret_cast<double *>(Bs), &s_flag);
    }
}

__global__ void rank_finalize_kernel(const unsigned long long *__restrict__ best_key, int64_t n1,
                                     int32_t *__restrict__ argmax) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n1) argmax[i] = (int32_t)(0xFFFFFFFFu - (uint32_t)(best_key[i] & 0xFFFFFFFFull));
}

// ---- store epilogue: M = e1 rows (output rows), N = e2 rows (output columns) ----------------------
__global__ __launch_bounds__(256, 2) void sim_inner_store_kernel(const float *__restrict__ e1, int64_t n1, int ld1,
                                                              const float *__restrict__ e2, int64_t n2, int ld2,
                                                              int dim, float *__restrict__ out, int64_t ld_out,
                                                              const int32_t *__restrict__ gate) {
    __shared__ __attribute__((aligned(16))) float As[2 * TILE * LDS_LD];
    __shared__ __attribute__((aligned(16))) float Bs[2 * TILE * LDS_LD];
    if (gate && *gate == 0) return;          // device-side gate (the CSLS means' fallback strips: nothing failed)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int64_t m0 = (int64_t)blockIdx.y * TILE, c0 = (int64_t)blockIdx.x * TILE;
    tile_pipeline_packed(
        e1, ld1, e2, dim, c0, 1, [=](int64_t) { return m0; }, As, Bs,
        [&](int64_t, f32x16 (&acc)[2][2]) {
            float *tile = out + m0 * ld_out + c0;                                    // wave-uniform
            const int rows_left = (int)(n1 - m0 < TILE ? n1 - m0 : TILE), cols_left = (int)(n2 - c0 < TILE ? n2 - c0 : TILE);
            const int col = wn * 64 + (lane & 31), rbase = wm * 64 + 4 * (lane >> 5);
            const bool ok0 = col < cols_left, ok1 = col + 32 < cols_left;
#pragma unroll
            for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = rbase + tm * 32 + (r & 3) + 8 * (r >> 2);
                    if (row < rows_left) {
                        float *p = tile + (row * (int)ld_out + col);               // 128 rows * ld_out < 2^31
                        if (ok0) p[0] = acc[tm][0][r];
                        if (ok1) p[32] = acc[tm][1][r];
                    }
                    asm volatile("" ::: "memory");      // keep the 32 row addresses from all being live at once
                }
        });
}

// ---- fp64 VALU tiles: manhattan / euclidean --------------------------------------------------------
// 64 queries x 64 candidates per block, 4x4 per thread, K chunk 32 staged as doubles.
// sim = float(1 - sum_k |a_k - b_k|)  (scipy cdist cityblock, similarity.py:46-48), sequential k.
constexpr int VT = 64, VK = 32;

__device__ __forceinline__ void stage_f64(const float *__restrict__ src, int64_t n, int ld, int dim, int64_t row0,
                                          int k0, double *__restrict__ dst /* [VK][VT+1] */, int tid) {
    // thread -> (row = tid / 4, 8 k values starting at (tid % 4) * 8)
    const int r = tid >> 2, kq = (tid & 3) * 8;
    const int64_t row = row0 + r;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = k0 + kq + e;
        float v = 0.f;
        if (row < n && k < dim) v = src[row * ld + k];
        dst[(kq + e) * (VT + 1) + r] = (double)v;
    }
}

template <int METRIC>
__device__ __forceinline__ void valu_tile(const float *__restrict__ e1, int64_t n1, int ld1,
                                          const float *__restrict__ e2, int64_t n2, int ld2, int dim, int64_t q0,
                                          int64_t c0, double *Qs, double *Cs, float (&simv)[4][4]) {
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
    for (int k0 = 0; k0 < dim; k0 += VK) {
        __syncthreads();
        stage_f64(e1, n1, ld1, dim, q0, k0, Qs, tid);
        stage_f64(e2, n2, ld2, dim, c0, k0, Cs, tid);
        __syncthreads();
        const int kk = min(VK, dim - k0);
        for (int k = 0; k < kk; ++k) {
            double qv[4], cv[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) qv[a] = Qs[k * (VT + 1) + ty * 4 + a];
#pragma unroll
            for (int b = 0; b < 4; ++b) cv[b] = Cs[k * (VT + 1) + tx + 16 * b];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const double t = qv[a] - cv[b];
                    if (METRIC == OEA_METRIC_MANHATTAN) acc[a][b] += fabs(t);
                    else acc[a][b] += t * t;
                }
        }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
            simv[a][b] = METRIC == OEA_METRIC_MANHATTAN ? (float)(1.0 - acc[a][b]) : (float)(1.0 - sqrt(acc[a][b]));
}

template <int METRIC>
__global__ void gold_valu_kernel(const float *__restrict__ e1, int64_t n1, int ld1, const float *__restrict__ e2,
                                 int ld2, int dim, const float *__restrict__ csls_r,
                                 const float *__restrict__ csls_c, float *__restrict__ gold) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n1) return;
    const float *a = e1 + i * ld1, *b = e2 + i * ld2;
    double s = 0.0;
    for (int k = 0; k < dim; ++k) {
        const double t = (double)a[k] - (double)b[k];
        if (METRIC == OEA_METRIC_MANHATTAN) s += fabs(t);
        else s += t * t;
    }
    float v = METRIC == OEA_METRIC_MANHATTAN ? (float)(1.0 - s) : (float)(1.0 - sqrt(s));
    if (csls_r) v = (2.0f * v - csls_r[i]) - csls_c[i];
    gold[i] = v;
}

template <int METRIC>
__global__ __launch_bounds__(256) void rank_valu_kernel(
    const float *__restrict__ e1, int64_t n1, int ld1, const float *__restrict__ e2, int64_t n2, int ld2, int dim,
    const float *__restrict__ gold, const float *__restrict__ csls_r, const float *__restrict__ csls_c,
    int tiles_per_chunk, int64_t gold_off, int32_t *__restrict__ rank, unsigned long long *__restrict__ best_key) {
    __shared__ double Qs[VK * (VT + 1)];
    __shared__ double Cs[VK * (VT + 1)];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t q0 = (int64_t)blockIdx.x * VT;
    const int64_t nct = (n2 + VT - 1) / VT;
    const int64_t ct_begin = (int64_t)blockIdx.y * tiles_per_chunk;
    const int64_t ct_end = (ct_begin + tiles_per_chunk < nct) ? ct_begin + tiles_per_chunk : nct;
    int cnt[4] = {0, 0, 0, 0};
    float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    int bidx[4] = {0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff};
    float g[4], rq[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int64_t i = q0 + ty * 4 + a;
        g[a] = i < n1 ? gold[i] : 0.f;
        rq[a] = (i < n1 && csls_r) ? csls_r[i] : 0.f;
    }
    for (int64_t ct = ct_begin; ct < ct_end; ++ct) {
        const int64_t c0 = ct * VT;
        float simv[4][4];
        valu_tile<METRIC>(e1, n1, ld1, e2, n2, ld2, dim, q0, c0, Qs, Cs, simv);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int64_t j = c0 + tx + 16 * b;
            if (j < n2) {
                const float cj = csls_c ? csls_c[j] : 0.f;
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    const int64_t i = q0 + ty * 4 + a;
                    float v = simv[a][b];
                    if (csls_r) v = (2.0f * v - rq[a]) - cj;
                    cnt[a] += (j != i + gold_off) && (v > g[a] || (v == g[a] && j < i + gold_off));
                    if (v > best[a] || (v == best[a] && (int)j < bidx[a])) { best[a] = v; bidx[a] = (int)j; }
                }
            }
        }
    }
    if (ct_end > ct_begin) {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int64_t i = q0 + ty * 4 + a;
            if (i < n1) {
                if (cnt[a]) atomicAdd(rank + i, cnt[a]);
                const unsigned long long key = ((unsigned long long)f2ord(best[a]) << 32) | (0xFFFFFFFFu - (uint32_t)bidx[a]);
                atomicMax(best_key + i, key);
            }
        }
    }
}

// ---- L1 similarity in fp32 (pre-filter of RDGCN's hard-negative mining, rdgcn.py:75-87) ---------------------------------------
// 1 - sum |a - b| with fp32 accumulation: NOT the bits of scipy's cdist (that is sim_valu_store_kernel's fp64 chain, 92 ms for
// 20,000 x 200,000 x 300 at 0.68 of the fp64 vector peak); it only has to rank the candidates well enough that the true k
// nearest are among the k + margin it keeps -- those are then re-ranked with exact fp64 distances (oea_pair_l1_f64).
// 128 x 128 tile per workgroup, 8 x 8 outputs per thread: per k a thread reads its 8 + 8 operands with FOUR ds_read_b128
// (rows / columns t*4..+4 and 64 + t*4..+4: a 16-lane group reads 256 contiguous bytes, no bank conflict) for 128 vector
// operations -- the first version (64 x 64 tile, 4 x 4 outputs, 8 ds_read_b32 per 32 operations) spent as many LDS cycles as
// VALU cycles and was no faster than the fp64 kernel (88 vs 93 ms).  |.| is a free source modifier of the add.
constexpr int LT = 128, LK = 32;
__global__ __launch_bounds__(256) void sim_l1_f32_store_kernel(const float *__restrict__ e1, int64_t n1, int ld1,
                                                               const float *__restrict__ e2, int64_t n2, int ld2, int dim,
                                                               float *__restrict__ out, int64_t ld_out) {
    __shared__ __attribute__((aligned(16))) float Qs[LK * LT];
    __shared__ __attribute__((aligned(16))) float Cs[LK * LT];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t q0 = (int64_t)blockIdx.y * LT, c0 = (int64_t)blockIdx.x * LT;
    float acc[8][8];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) acc[a][b] = 0.f;
    // staging: thread -> (row = tid / 2, 16 k values starting at (tid % 2) * 16), stored k-major: [k][row]
    const int r = tid >> 1, kq = (tid & 1) * 16;
    for (int k0 = 0; k0 < dim; k0 += LK) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 16; e += 4) {
            const int k = k0 + kq + e;
            float4 qv = make_float4(0.f, 0.f, 0.f, 0.f), cv = make_float4(0.f, 0.f, 0.f, 0.f);
            if (q0 + r < n1 && k < ld1) qv = oea::ld4(e1 + (q0 + r) * ld1 + k);          // ld % 4 == 0; pad columns are zero
            if (c0 + r < n2 && k < ld2) cv = oea::ld4(e2 + (c0 + r) * ld2 + k);
            if (k + 0 >= dim) { qv.x = 0.f; cv.x = 0.f; }
            if (k + 1 >= dim) { qv.y = 0.f; cv.y = 0.f; }
            if (k + 2 >= dim) { qv.z = 0.f; cv.z = 0.f; }
            if (k + 3 >= dim) { qv.w = 0.f; cv.w = 0.f; }
            Qs[(kq + e + 0) * LT + r] = qv.x; Qs[(kq + e + 1) * LT + r] = qv.y; Qs[(kq + e + 2) * LT + r] = qv.z; Qs[(kq + e + 3) * LT + r] = qv.w;
            Cs[(kq + e + 0) * LT + r] = cv.x; Cs[(kq + e + 1) * LT + r] = cv.y; Cs[(kq + e + 2) * LT + r] = cv.z; Cs[(kq + e + 3) * LT + r] = cv.w;
        }
        __syncthreads();
        const int kk = min(LK, dim - k0);
        for (int k = 0; k < kk; ++k) {
            const float4 qa = *reinterpret_cast<const float4 *>(Qs + k * LT + ty * 4);
            const float4 qb = *reinterpret_cast<const float4 *>(Qs + k * LT + 64 + ty * 4);
            const float4 ca = *reinterpret_cast<const float4 *>(Cs + k * LT + tx * 4);
            const float4 cb = *reinterpret_cast<const float4 *>(Cs + k * LT + 64 + tx * 4);
            const float qv[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
            const float cv[8] = {ca.x, ca.y, ca.z, ca.w, cb.x, cb.y, cb.z, cb.w};
#pragma unroll
            for (int a = 0; a < 8; ++a)
#pragma unroll
                for (int b = 0; b < 8; ++b) acc[a][b] += fabsf(qv[a] - cv[b]);
        }
    }
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        const int64_t i = q0 + (a < 4 ? ty * 4 + a : 64 + ty * 4 + (a - 4));
        if (i >= n1) continue;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int64_t j = c0 + h * 64 + tx * 4;
            float *o = out + i * ld_out + j;
            if (j + 3 < n2 && (ld_out & 3) == 0) {
                oea::st4(o, make_float4(1.0f - acc[a][h * 4 + 0], 1.0f - acc[a][h * 4 + 1], 1.0f - acc[a][h * 4 + 2], 1.0f - acc[a][h * 4 + 3]));
            } else {
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (j + b < n2) o[b] = 1.0f - acc[a][h * 4 + b];
            }
        }
    }
}

template <int METRIC>
__global__ __launch_bounds__(256) void sim_valu_store_kernel(const float *__restrict__ e1, int64_t n1, int ld1,
                                                             const float *__restrict__ e2, int64_t n2, int ld2,
                                                             int dim, float *__restrict__ out, int64_t ld_out) {
    __shared__ double Qs[VK * (VT + 1)];
    __shared__ double Cs[VK * (VT + 1)];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t q0 = (int64_t)blockIdx.y * VT, c0 = (int64_t)blockIdx.x * VT;
    float simv[4][4];
    valu_tile<METRIC>(e1, n1, ld1, e2, n2, ld2, dim, q0, c0, Qs, Cs, simv);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int64_t i = q0 + ty * 4 + a, j = c0 + tx + 16 * b;
            if (i < n1 && j < n2) out[i * ld_out + j] = simv[a][b];
        }
}

// ---- integer metric reductions ---------------------------------------------------------------------
// hits[k] = #{rank < top_k[k]}, rank_sum = sum(rank + 1), rr_sum = sum 1/(rank+1) in a fixed order
// (one block, strided partials, tree reduce) -> deterministic.
__global__ __launch_bounds__(1024) void rank_metrics_kernel(const int32_t *__restrict__ rank, int64_t n, int4 tk0,
                                                            int4 tk1, int nk, long long *__restrict__ hits,
                                                            long long *__restrict__ rank_sum, double *__restrict__ rr_sum) {
    __shared__ long long s_i[1024];
    __shared__ double s_d[1024];
    const int tks[8] = {tk0.x, tk0.y, tk0.z, tk0.w, tk1.x, tk1.y, tk1.z, tk1.w};
    long long h[8] = {0, 0, 0, 0, 0, 0, 0, 0}, rs = 0;
    double rr = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
        const int r = rank[i];
#pragma unroll
        for (int k = 0; k < 8; ++k) h[k] += (k < nk && r < tks[k]);
        rs += r + 1;
        rr += 1.0 / (double)(r + 1);
    }
    // wave butterflies (fixed pairing), then the 16 wave results in wave order: deterministic, two barriers in all
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long v[9];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = h[k];
    v[8] = rs;
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) rr += __shfl_xor(rr, off, 64);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) s_i[wave * 9 + k] = v[k];
        s_d[wave] = rr;
    }
    __syncthreads();
    if (threadIdx.x <= 9) {
        const int nw = blockDim.x >> 6;
        if (threadIdx.x < 9) {
            long long t = 0;
            for (int w = 0; w < nw; ++w) t += s_i[w * 9 + threadIdx.x];
            if ((int)threadIdx.x < nk) hits[threadIdx.x] = t;
            else if (threadIdx.x == 8) *rank_sum = t;
        } else {
            double t = 0.0;
            for (int w = 0; w < nw; ++w) t += s_d[w];
            *rr_sum = t;
        }
    }
}

// ---- rank of given gold columns on an explicit similarity block (calculate_rank, alignment.py:146-168)
// one workgroup per row: rank = #{S_ij > S_ig} + #{j < g : S_ij == S_ig}, argmax = smallest j of the max
__global__ __launch_bounds__(256) void rank_rows_kernel(const float *__restrict__ s, int64_t nc, int64_t ld,
                                                        const int32_t *__restrict__ gold_idx, int32_t *__restrict__ rank,
                                                        int32_t *__restrict__ argmax) {
    __shared__ int s_cnt[4];
    __shared__ unsigned long long s_key[4];
    const int64_t row = blockIdx.x;
    const float *src = s + row * ld;
    const int g = gold_idx[row];
    const float gv = src[g];
    int cnt = 0;
    unsigned long long best = 0ull;
    for (int64_t j = threadIdx.x; j < nc; j += 256) {
        const float v = src[j];
        cnt += (j != g) && (v > gv || (v == gv && j < g));
        const unsigned long long key = ((unsigned long long)f2ord(v) << 32) | (0xFFFFFFFFu - (uint32_t)j);
        best = key > best ? key : best;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        cnt += __shfl_xor(cnt, off, 64);
        const unsigned long long o = __shfl_xor(best, off, 64);
        best = o > best ? o : best;
    }
    if ((threadIdx.x & 63) == 0) { s_cnt[threadIdx.x >> 6] = cnt; s_key[threadIdx.x >> 6] = best; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
        unsigned long long b = 0ull;
        for (int w = 0; w < 4; ++w) { c += s_cnt[w]; b = s_key[w] > b ? s_key[w] : b; }
        rank[row] = c;
        argmax[row] = (int32_t)(0xFFFFFFFFu - (uint32_t)(b & 0xFFFFFFFFull));
    }
}

// ---- certified bf16 prefilter for the inner-product rank sweep (round 4) ------------------------------------------------------
// The exact evaluation multiplies in fp32 (v_mfma_f32_32x32x2_f32: 1/16 of the bf16 matrix rate).  Here every operand is split
// x = hi + lo + r (hi = bf16(x), lo = bf16(x - hi), |r| <= 2^-18 |x|) and the tile sweep accumulates hi.hi + hi.lo + lo.hi with
// v_mfma_f32_32x32x16_bf16 -- 3/16 of the fp32 pipe time, the same LDS bytes (hi + lo = 4 B per element).  The result v~ is
// within tol = eps(dim) |q|max |c|max of the exact k-ordered fmaf chain v (split residue 3 * 2^-18, fp32 accumulation of
// 3 * Kp products bounded term by term, the chain's own rounding).  So against the exact gold value g:
//     v~ > g + tol   certainly greater: counted in the sweep;      v~ < g - tol   certainly smaller: ignored;
//     |v~ - g| <= tol                 a RECORD (query, candidate): decided afterwards by the exact chain, tie rule included;
// and the nearest candidate: a candidate can only be the exact row maximum if v~ + tol >= (the best lower bound v~' - tol seen
// so far, gold included), so those are recorded too (the bound is shared by the lanes of a row through an atomic maximum).
// The fix-up kernel evaluates the records -- a few dozen per row -- exactly.  Ranks and nearest candidates are those of the
// fp32 sweep, bit for bit; if the record buffer overflows the caller takes the fp32 sweep.

constexpr uint32_t kRecTop = 0x80000000u;        // record kinds: bit 31 of the candidate word

// gold, tolerance, per-row state of the bf16 sweep
// nmax: float bits of max |e1 row|, max |e2 row|, max |csls_c|
__global__ void rank_bf16_init_kernel(const float *__restrict__ gold, int64_t n1, int64_t gold_off, const unsigned *__restrict__ nmax,
                                      float eps_rel, const float *__restrict__ csls_r, float *__restrict__ tol_out,
                                      int32_t *__restrict__ rank, unsigned long long *__restrict__ best_key,
                                      unsigned *__restrict__ lbrow, unsigned *__restrict__ rec_cnt) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const float smax = __uint_as_float(nmax[0]) * __uint_as_float(nmax[1]);
    // + an absolute slack for the ulp-level roundings of g +- tol, v~ - tol and of the comparisons themselves (values <= smax)
    const float tol0 = 1.05f * eps_rel * smax + 1.0e-6f * smax + 1e-30f;
    const float scale = 2.0f * smax + __uint_as_float(nmax[2]) + 2.0f * tol0;
    if (i == 0) { tol_out[0] = tol0; tol_out[1] = scale; rec_cnt[0] = 0u; rec_cnt[1] = 0u; }
    if (i >= n1) return;
    const float tol = csls_r ? 2.0f * tol0 + 3.0e-7f * (scale + fabsf(csls_r[i])) : tol0;      // == the sweep's per-lane tolerance
    rank[i] = 0;
    best_key[i] = ((unsigned long long)f2ord(gold[i]) << 32) | (0xFFFFFFFFu - (uint32_t)(i + gold_off));     // the gold is a candidate
    lbrow[i] = f2ord(gold[i] - tol);
}

// WARM: a first pass over the first `tiles_per_chunk` candidate tiles only raises the rows' lower bounds (lbrow = max v~ - tol
// over a few thousand candidates: about the (n2 / 2048)-th largest value of the row), so that the full sweep records as
// nearest-candidate suspects only the few dozen candidates above that -- without it a row whose gold is far from the top
// records every running maximum of every lane (hundreds per row).
// Records go to a slice of the record buffer PRIVATE to the wave (slot = count + prefix of a ballot; no returning atomic:
// the first version took one global round trip per recording wave instruction and ran 4x slower on rows whose gold is far
// from the top).  rec_cnt[2 + wave id] = the slice's length; a full slice raises the overflow flag.
// CSLS: the values compared are (2 s - r_i) - c_j (rank_inner_kernel's expression on the approximate s); tol[tn] then holds
// 2 tol + the rounding slack of the two extra operations for this lane's query.
// The three classes are COMPLEMENTARY comparisons against ghi = g + tol and glo = g - tol (counted: v > ghi; band: glo <= v <=
// ghi; ignored: v < glo) -- a first version tested the band as |v - g| <= tol, whose rounding left a gap of an ulp below ghi
// through which one candidate in ~10^7 fell.  The ulp-level roundings of g +- tol themselves sit inside the absolute slack
// of the tolerance (rank_bf16_init_kernel).
template <bool WARM, bool INTERIOR, bool CSLS, class Acc, class Rec>
__device__ __forceinline__ void rank_bf16_tile(Acc &acc, int jb, int n2, const float (&glo)[2], const float (&ghi)[2], float (&lb)[2],
                                               float (&lbm)[2], int (&cnt)[2], bool (&dirty)[2], const int64_t (&qi)[2], int64_t gold_off,
                                               const float (&tol)[2], const float (&rq)[2], float my_c, Rec &&record) {
    // my_c: the column mean of the candidate this lane looks after (lane l32 = tm * 16 + r of either half: one load per tile and
    // lane + a lane shuffle per register instead of 32 loaded values held in registers)
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int tm = 0; tm < 2; ++tm) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = jb + tm * 32 + (r & 3) + 8 * (r >> 2);
            const bool jin = INTERIOR || j < n2;
            const float cj = CSLS ? __shfl(my_c, (lane & 32) + tm * 16 + r, 64) : 0.f;
#pragma unroll
            for (int tn = 0; tn < 2; ++tn) {
                float v = acc[tm][tn][r];
                if (CSLS) v = fmaf(2.0f, v, -rq[tn]) - cj;
                if (WARM) {
                    if (jin) lb[tn] = fmaxf(lb[tn], v - tol[tn]);
                    continue;
                }
                cnt[tn] += (v > ghi[tn]) & jin;
                const bool band = (v <= ghi[tn]) & (v >= glo[tn]);
                const bool hit = ((v >= lbm[tn]) | band) & jin;
                if (__ballot(hit)) {                                  // wave-uniform branch: rare
                    const bool other = hit && (int64_t)j != qi[tn] + gold_off;
                    record(other && v >= lbm[tn], tn, j, kRecTop);
                    record(other && band, tn, j, 0u);
                    if (hit && v - tol[tn] > lb[tn]) { lb[tn] = v - tol[tn]; lbm[tn] = lb[tn] - tol[tn]; dirty[tn] = true; }
                }
            }
        }
    }
}

// NCH = 0: both operands through LDS (tile_pipeline_bf16, any Kp); NCH = Kp / 32 in {1..4}: B in registers (tile_pipeline_bf16_breg);
// NW = 8: 512 threads on 256-candidate tiles through the three-stage ring (tile_pipeline_bf16_big<PF>; tiles_per_chunk counts THOSE
// tiles)
template <bool WARM, bool CSLS, int NCH, int NW = 4, bool PF = true>
__device__ __forceinline__ void rank_bf16_body(
    const float *__restrict__ qp, int64_t n1, int kp, const float *__restrict__ cp, int64_t n2, int dim,
    const float *__restrict__ gold, const float *__restrict__ tol_ptr, const float *__restrict__ csls_r,
    const float *__restrict__ csls_c, int tiles_per_chunk, int64_t gold_off,
    int32_t *__restrict__ rank, unsigned *__restrict__ lbrow, uint2 *__restrict__ rec, unsigned *__restrict__ rec_cnt, unsigned slice_cap,
    TileGrid tg, float *As, float *Bs) {
    unsigned bx, by;
    if (!tile_grid_item(tg, bx, by)) return;               // (the whole workgroup: padding of the XCD-aware launch)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int64_t q0 = (int64_t)bx * TILE;
    constexpr int MT = NW * 32;                              // candidate rows of a tile
    const int64_t nct = (n2 + MT - 1) / MT;
    const int64_t ct_begin = (int64_t)by * tiles_per_chunk;
    const int64_t ct_end = (ct_begin + tiles_per_chunk < nct) ? ct_begin + tiles_per_chunk : nct;
    const float tol0 = tol_ptr[0];                         // bound on |s~ - s|; tol_ptr[1] = slack scale of the CSLS expression
    const unsigned wid = (by * tg.nx + bx) * (unsigned)NW + (unsigned)wave;
    uint2 *__restrict__ my_rec = rec + (size_t)wid * slice_cap;
    unsigned nrec = 0;                                     // wave-uniform
    int64_t qi[2];
    float glo[2], ghi[2], lb[2], lbm[2], tol[2], rq[2];
    int cnt[2] = {0, 0};
    bool dirty[2] = {false, false};
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
        qi[tn] = q0 + wn * 64 + tn * 32 + (lane & 31);
        const bool ok = qi[tn] < n1;
        const float g = ok ? gold[qi[tn]] : INFINITY;      // padding rows: nothing counts, nothing is recorded
        rq[tn] = (CSLS && ok) ? csls_r[qi[tn]] : 0.f;
        // (2 s~ - r) - c against (2 s - r) - c: twice the bound on s, plus the roundings of the fma and of the subtraction on
        // either side (each <= 2^-24 of a value <= 2 |s|max + |r| + |c|max = tol_ptr[1] + |r|)
        tol[tn] = CSLS ? 2.0f * tol0 + 3.0e-7f * (tol_ptr[1] + fabsf(rq[tn])) : tol0;
        ghi[tn] = g + tol[tn];
        glo[tn] = ok ? g - tol[tn] : INFINITY;
        lb[tn] = glo[tn];
        lbm[tn] = lb[tn] - tol[tn];
    }
    auto record = [&](bool pred, int tn, int j, uint32_t kind) {
        const unsigned long long m = __ballot(pred);
        if (m == 0ull) return;
        const unsigned at = nrec + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
        if (pred && at < slice_cap) my_rec[at] = make_uint2((uint32_t)qi[tn], (uint32_t)j | kind);
        nrec += (unsigned)__popcll(m);
    };
    // what a tile's epilogue reads from memory -- the row's shared bound (other lanes / workgroups may have raised it) and, with CSLS,
    // the column mean this lane looks after -- is requested ONE TILE AHEAD (round 6): asked for at the top of the epilogue it was an
    // exposed L2 round trip per tile and wave.  A bound that is one tile old is still a lower bound (it only grows).
    const int l32c = lane & 31;
    const int my_off = wm * 64 + 4 * (lane >> 5) + (l32c >> 4) * 32 + (l32c & 3) + 8 * ((l32c & 15) >> 2);
    unsigned lb_pre[2] = {0u, 0u};
    float c_pre = 0.f;
    auto prefetch = [&](int64_t t) {                         // for tile t of this work item
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
            if (qi[tn] < n1) lb_pre[tn] = __hip_atomic_load(lbrow + qi[tn], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (CSLS) {
            const int64_t my_j = (ct_begin + t) * MT + my_off;
            c_pre = (my_j < n2 && ct_begin + t < ct_end) ? csls_c[my_j] : 0.f;
        }
    };
    prefetch(0);
    auto epilogue = [&](int64_t t, f32x16 (&acc)[2][2]) {
            const int64_t c0 = (ct_begin + t) * MT;
            const int jb = (int)c0 + wm * 64 + 4 * (lane >> 5);
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
                if (qi[tn] < n1) {
                    const float o = ord2f(lb_pre[tn]);
                    if (o > lb[tn]) { lb[tn] = o; lbm[tn] = o - tol[tn]; }
                }
            const float my_c = CSLS ? c_pre : 0.f;
            prefetch(t + 1);
            if (c0 + MT <= n2) rank_bf16_tile<WARM, true, CSLS>(acc, jb, (int)n2, glo, ghi, lb, lbm, cnt, dirty, qi, gold_off, tol, rq, my_c, record);
            else rank_bf16_tile<WARM, false, CSLS>(acc, jb, (int)n2, glo, ghi, lb, lbm, cnt, dirty, qi, gold_off, tol, rq, my_c, record);
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
                if (dirty[tn]) { atomicMax(lbrow + qi[tn], f2ord(lb[tn])); dirty[tn] = false; }
        };
    auto m_tile = [=](int64_t t) { return (ct_begin + t) * MT; };
    const int64_t n_tiles = ct_end > ct_begin ? ct_end - ct_begin : 0;
    if constexpr (NW == 8) tile_pipeline_bf16_big<PF>(cp, kp, qp, dim, q0, n_tiles, m_tile, As, epilogue);
    else if constexpr (NCH > 0) tile_pipeline_bf16_breg<NCH>(cp, kp, qp, q0, n_tiles, m_tile, As, epilogue, dim);
    else tile_pipeline_bf16<true>(cp, kp, qp, dim, q0, n_tiles, m_tile, As, Bs, epilogue);
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
        if (WARM) {
            lb[tn] = fmaxf(lb[tn], __shfl_xor(lb[tn], 32, 64));
            if (lane < 32 && qi[tn] < n1) atomicMax(lbrow + qi[tn], f2ord(lb[tn]));
            continue;
        }
        cnt[tn] += __shfl_xor(cnt[tn], 32, 64);
        if (lane < 32 && qi[tn] < n1 && cnt[tn]) atomicAdd(rank + qi[tn], cnt[tn]);
    }
    if (!WARM && lane == 0) {
        rec_cnt[2 + wid] = min(nrec, slice_cap);
        if (nrec) atomicAdd(rec_cnt, nrec);                   // total (statistics)
        if (nrec > slice_cap) atomicMax(rec_cnt + 1, 1u);     // overflow: the caller falls back to the fp32 sweep
    }
}

#define OEA_RANK_BF16_PARAMS                                                                                                        \
    const float *__restrict__ qp, int64_t n1, int kp, const float *__restrict__ cp, int64_t n2, int dim,                            \
    const float *__restrict__ gold, const float *__restrict__ tol_ptr, const float *__restrict__ csls_r,                            \
    const float *__restrict__ csls_c, int tiles_per_chunk, int64_t gold_off, int32_t *__restrict__ rank,                            \
    unsigned *__restrict__ lbrow, uint2 *__restrict__ rec, unsigned *__restrict__ rec_cnt, unsigned slice_cap, TileGrid tg
#define OEA_RANK_BF16_ARGS qp, n1, kp, cp, n2, dim, gold, tol_ptr, csls_r, csls_c, tiles_per_chunk, gold_off, rank, lbrow, rec, rec_cnt, slice_cap, tg

template <bool WARM, bool CSLS>
__global__ __launch_bounds__(256, 2) void rank_bf16_kernel(OEA_RANK_BF16_PARAMS) {
    __shared__ __attribute__((aligned(16))) float As[2 * TILE * LDS_LD];
    __shared__ __attribute__((aligned(16))) float Bs[2 * TILE * LDS_LD];
    rank_bf16_body<WARM, CSLS, 0>(OEA_RANK_BF16_ARGS, As, Bs);
}

template <bool WARM, bool CSLS, int NCH>
__global__ __launch_bounds__(256, 2) void rank_bf16_breg_kernel(OEA_RANK_BF16_PARAMS) {
    __shared__ __attribute__((aligned(16))) float As[4 * TILE * PLD];           // 2 slots x 2 chunks
    rank_bf16_body<WARM, CSLS, NCH>(OEA_RANK_BF16_ARGS, As, nullptr);
}

template <bool CSLS, bool PF>
__global__ __launch_bounds__(512, 2) void rank_bf16_big_kernel(OEA_RANK_BF16_PARAMS) {
    extern __shared__ __attribute__((aligned(16))) float big_lds[];                // BIG_LDS_BYTES
    rank_bf16_body<false, CSLS, 0, 8, PF>(OEA_RANK_BF16_ARGS, big_lds, nullptr);
}

// ONE grid-stride prologue: both bf16 packs, the gold similarities (the exact k-ordered chain), the max row norms of both
// tables, zeroing of ranks / counters
__global__ __launch_bounds__(256) void rank_bf16_prologue_kernel(const float *__restrict__ e1, int64_t n1, int ld1,
                                                                 const float *__restrict__ e2, int64_t n2, int ld2, int dim,
                                                                 int64_t gold_off, uint4 *__restrict__ p1, int64_t n1_pad,
                                                                 uint4 *__restrict__ p2, int64_t n2_pad, int kp,
                                                                 float *__restrict__ gold, unsigned *__restrict__ nmax,
                                                                 int32_t *__restrict__ rank, const float *__restrict__ csls_r,
                                                                 const float *__restrict__ csls_c, int aug) {
    // aug (with the CSLS means): the packed rows carry two more coordinates, q' = [2 q, -r_i, -1] and c' = [c, 1, c_j], so that the
    // tile sweep's product IS 2 <q, c> - r_i - c_j and the sweep runs without the CSLS terms in its epilogue (same kernel, same
    // registers as the plain evaluation); the norms below are those of the augmented rows
    const int cpr = kp / 4;
    const int64_t a_end = n1_pad * cpr, b_end = a_end + n2_pad * cpr;
    // then: the gold chains (one thread per query row), then the row norms (16 lanes per row, table 2 on a wave boundary)
    const int64_t g_end = b_end + (n1 + 63) / 64 * 64;
    const int64_t m1_end = g_end + (16 * n1 + 63) / 64 * 64, m2_end = m1_end + (16 * n2 + 63) / 64 * 64;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m2_end; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < b_end) {
            const bool second = i >= a_end;
            const int64_t li = second ? i - a_end : i;
            const float *src = second ? e2 : e1;
            const int64_t n = second ? n2 : n1;
            const int ld = second ? ld2 : ld1;
            const int64_t row = li / cpr;
            const int c = (int)(li - row * cpr);
            const int g = c & 7, k0 = 32 * (c >> 3) + 16 * (g >> 2) + 8 * ((g >> 1) & 1), lo = g & 1;
            uint32_t h[8];
            float x[8];
            if (row < n && k0 + 8 <= dim) {
                const float4 u = oea::ld4(src + row * ld + k0), w = oea::ld4(src + row * ld + k0 + 4);
                x[0] = u.x; x[1] = u.y; x[2] = u.z; x[3] = u.w; x[4] = w.x; x[5] = w.y; x[6] = w.z; x[7] = w.w;
            } else {
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    x[t] = (row < n && k0 + t < dim) ? src[row * ld + k0 + t] : 0.f;
                    if (aug && row < n && k0 + t == dim) x[t] = second ? 1.0f : -csls_r[row];
                    if (aug && row < n && k0 + t == dim + 1) x[t] = second ? csls_c[row] : -1.0f;
                }
            }
            if (aug && !second) {
#pragma unroll
                for (int t = 0; t < 8; ++t)
                    if (k0 + t < dim) x[t] *= 2.0f;                   // exact
            }
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const uint32_t hi = bf16_rne(x[t]);
                h[t] = lo ? bf16_rne(x[t] - __uint_as_float(hi << 16)) : hi;
            }
            (second ? p2 : p1)[li] = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
            continue;
        }
        if (i < g_end) {
            const int64_t row = i - b_end;
            if (row < n1) {
                const float *a = e1 + row * ld1, *b = e2 + (row + gold_off) * ld2;
                float acc = 0.f;
                int k = 0;
                for (; k + 4 <= dim; k += 4) {
                    const float4 x = oea::ld4(a + k), y = oea::ld4(b + k);
                    acc = fmaf(x.x, y.x, acc); acc = fmaf(x.y, y.y, acc); acc = fmaf(x.z, y.z, acc); acc = fmaf(x.w, y.w, acc);
                }
                for (; k < dim; ++k) acc = fmaf(a[k], b[k], acc);
                if (csls_r) acc = (2.0f * acc - csls_r[row]) - csls_c[row + gold_off];       // gold_inner_kernel's expression
                gold[row] = acc;
                rank[row] = 0;
            }
            continue;
        }
        const bool second = i >= m1_end;
        const int64_t li = second ? i - m1_end : i - g_end;
        const int64_t row = li >> 4, n = second ? n2 : n1;
        const int l16 = (int)(li & 15);
        float ss = 0.f;
        if (row < n) {
            const float *a = second ? e2 + row * ld2 : e1 + row * ld1;
            for (int k = l16; k < dim; k += 16) ss = fmaf(a[k], a[k], ss);
        }
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);
        if (aug && row < n) {
            const float extra = second ? csls_c[row] : csls_r[row];
            ss = (second ? ss : 4.0f * ss) + fmaf(extra, extra, 1.0f);
        }
        float nr = sqrtf(ss) * 1.000001f;
        float cm = (second && csls_c && row < n && l16 == 0) ? fabsf(csls_c[row]) : 0.f;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            nr = fmaxf(nr, __shfl_xor(nr, off, 64));
            cm = fmaxf(cm, __shfl_xor(cm, off, 64));
        }
        if ((threadIdx.x & 63) == 0 && cm > __uint_as_float(__hip_atomic_load(nmax + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)))
            atomicMax(nmax + 2, __float_as_uint(cm));
        // one atomic per wave, and only when it would raise the maximum (35,000 waves on two addresses took 0.3 ms)
        unsigned *dst = nmax + (second ? 1 : 0);
        if ((threadIdx.x & 63) == 0 && nr > __uint_as_float(__hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)))
            atomicMax(dst, __float_as_uint(nr));
    }
}

// argmax from the keys + Hits@k / sum(rank + 1) / sum 1 / (rank + 1) in a fixed order + the sweep's status, ONE block
__global__ __launch_bounds__(1024) void rank_bf16_finish_kernel(const int32_t *__restrict__ rank, const unsigned long long *__restrict__ best_key,
                                                                int64_t n, int4 tk0, int4 tk1, int nk, int32_t *__restrict__ argmax,
                                                                long long *__restrict__ out, const unsigned *__restrict__ rec_cnt) {
    __shared__ long long s_i[1024];
    __shared__ double s_d[1024];
    const int tks[8] = {tk0.x, tk0.y, tk0.z, tk0.w, tk1.x, tk1.y, tk1.z, tk1.w};
    long long h[8] = {0, 0, 0, 0, 0, 0, 0, 0}, rs = 0;
    double rr = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
        const int r = rank[i];
        argmax[i] = (int32_t)(0xFFFFFFFFu - (uint32_t)(best_key[i] & 0xFFFFFFFFull));
#pragma unroll
        for (int k = 0; k < 8; ++k) h[k] += (k < nk && r < tks[k]);
        rs += r + 1;
        rr += 1.0 / (double)(r + 1);
    }
    // the reduction order of rank_metrics_kernel (wave butterflies, then the wave results in wave order): the same bits
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long v[9];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = h[k];
    v[8] = rs;
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) rr += __shfl_xor(rr, off, 64);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) s_i[wave * 9 + k] = v[k];
        s_d[wave] = rr;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int nw = blockDim.x >> 6;
        for (int k = 0; k < 9; ++k) {
            long long t = 0;
            for (int w = 0; w < nw; ++w) t += s_i[w * 9 + k];
            if (k < nk) out[k] = t;
            else if (k == 8) out[nk] = t;
        }
        double t = 0.0;
        for (int w = 0; w < nw; ++w) t += s_d[w];
        out[nk + 1] = __double_as_longlong(t);
        out[nk + 2] = rec_cnt[1];            // != 0: the record buffer overflowed, nothing above is valid
        out[nk + 3] = rec_cnt[0];
    }
}

// the records by the exact k-ordered fmaf chain (gold_inner_kernel's arithmetic): one thread per record, workgroups
// stride over the waves' slices
__global__ __launch_bounds__(256) void rank_bf16_fixup_kernel(const float *__restrict__ e1, int ld1, const float *__restrict__ e2, int ld2,
                                                              int dim, const float *__restrict__ gold, int64_t gold_off,
                                                              const float *__restrict__ csls_r, const float *__restrict__ csls_c,
                                                              const uint2 *__restrict__ rec, const unsigned *__restrict__ rec_cnt,
                                                              unsigned n_slices, unsigned slice_cap, int32_t *__restrict__ rank,
                                                              unsigned long long *__restrict__ best_key) {
    if (rec_cnt[0] == 0u) return;
    const int sub = threadIdx.x >> 6, lane = threadIdx.x & 63;          // one wave per slice at a time
    for (unsigned sl = blockIdx.x * 4u + sub; sl < n_slices; sl += gridDim.x * 4u) {
        const unsigned n = rec_cnt[2 + sl];
        for (unsigned p = lane; p < n; p += 64) {
            const uint2 rc = rec[(size_t)sl * slice_cap + p];
            const int64_t i = rc.x, j = rc.y & 0x7FFFFFFFu;
            const float *a = e1 + i * ld1, *b = e2 + j * ld2;
            float acc = 0.f;
            int k = 0;
            for (; k + 32 <= dim; k += 32) {                        // 16 loads in flight, then the chain in k order
                float4 x[8], y[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) { x[u] = oea::ld4(a + k + 4 * u); y[u] = oea::ld4(b + k + 4 * u); }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    acc = fmaf(x[u].x, y[u].x, acc); acc = fmaf(x[u].y, y[u].y, acc);
                    acc = fmaf(x[u].z, y[u].z, acc); acc = fmaf(x[u].w, y[u].w, acc);
                }
            }
            for (; k + 4 <= dim; k += 4) {
                const float4 x = oea::ld4(a + k), y = oea::ld4(b + k);
                acc = fmaf(x.x, y.x, acc); acc = fmaf(x.y, y.y, acc); acc = fmaf(x.z, y.z, acc); acc = fmaf(x.w, y.w, acc);
            }
            for (; k < dim; ++k) acc = fmaf(a[k], b[k], acc);
            if (csls_r) acc = fmaf(2.0f, acc, -csls_r[i]) - csls_c[j];                // rank_inner_kernel's expression
            if (rc.y & kRecTop) {
                atomicMax(best_key + i, ((unsigned long long)f2ord(acc) << 32) | (0xFFFFFFFFu - (uint32_t)j));
            } else {
                const float gi = gold[i];
                if (acc > gi || (acc == gi && j < i + gold_off)) atomicAdd(rank + i, 1);
            }
        }
    }
}

// the approximate similarities themselves (tests: the error bound; timing of the bare sweep)
__global__ __launch_bounds__(256, 2) void sim_bf16_store_kernel(const float *__restrict__ e1p, int64_t n1, int kp,
                                                               const float *__restrict__ e2p, int64_t n2, int dim,
                                                               float *__restrict__ out, int64_t ld_out) {
    __shared__ __attribute__((aligned(16))) float As[2 * TILE * LDS_LD];
    __shared__ __attribute__((aligned(16))) float Bs[2 * TILE * LDS_LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int64_t m0 = (int64_t)blockIdx.y * TILE, c0 = (int64_t)blockIdx.x * TILE;
    tile_pipeline_bf16<true>(
        e1p, kp, e2p, dim, c0, 1, [=](int64_t) { return m0; }, As, Bs,
        [&](int64_t, f32x16 (&acc)[2][2]) {
            float *tile = out + m0 * ld_out + c0;
            const int rows_left = (int)(n1 - m0 < TILE ? n1 - m0 : TILE), cols_left = (int)(n2 - c0 < TILE ? n2 - c0 : TILE);
            const int col = wn * 64 + (lane & 31), rbase = wm * 64 + 4 * (lane >> 5);
            const bool ok0 = col < cols_left, ok1 = col + 32 < cols_left;
#pragma unroll
            for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = rbase + tm * 32 + (r & 3) + 8 * (r >> 2);
                    if (row < rows_left) {
                        float *p = tile + (row * (int)ld_out + col);
                        if (ok0) p[0] = acc[tm][0][r];
                        if (ok1) p[32] = acc[tm][1][r];
                    }
                    asm volatile("" ::: "memory");
                }
        });
}

// tol[0] = bound on |v~ - v| of the neighbour search's bf16 sweep from tol[1] = bits of the max row norm (as rank_bf16_init_kernel)
__global__ void knn_tol_kernel(float *tol, float eps_rel) {
    const float nm = tol[1], smax = nm * nm;
    tol[0] = 1.05f * eps_rel * smax + 1.0e-6f * smax + 1e-30f;
}

// tol[0] = bound on |v~ - v| of the CSLS means' bf16 sweep from tol[1], tol[2] = bits of the max row norms of the two tables
__global__ void csls_tol_kernel(float *tol, float eps_rel) {
    const float smax = tol[1] * tol[2];
    tol[0] = 1.05f * eps_rel * smax + 1.0e-6f * smax + 1e-30f;
}

// Two grow-only scratch slots (one per operand) instead of an allocation per call: at 10,500^2 two stream-ordered
// allocations + frees cost 0.12 ms on a 0.37 ms evaluation.  Reuse is ordered by the stream; a call on ANOTHER stream
// first waits for the event recorded after the previous use.  Growing a slot frees the old one (hipFree waits for the
// device), so kernels still reading it are done.
struct PackSlot {
    float *p = nullptr;
    size_t cap = 0;
    hipStream_t last = nullptr;
    hipEvent_t used = nullptr;
};
static PackSlot g_slot[6];       // 0 = queries, 1 = candidates, 2 / 3 = column / row samples (neighbour search, CSLS means),
                                 // 3 also = the bf16 split rows of the neighbour search, 4 / 5 = the bf16 split operands of the CSLS means

}  // namespace

// ---- host side of the packed path: what sim_tiles.h declares ---------------------------------------------------------------------
namespace oea {

int pick_chunks(int64_t q_tiles, int64_t c_tiles, int *tiles_per_chunk) {
    // enough workgroups to fill 256 CUs several times over, without splitting finer than a tile
    // (OEA_RANK_WGS overrides the target count: experiments)
    static const int64_t target = [] { const char *e = getenv("OEA_RANK_WGS"); return e ? (int64_t)atoi(e) : (int64_t)3072; }();
    int64_t want = std::max<int64_t>(1, (target + q_tiles - 1) / q_tiles);
    int64_t chunks = std::min<int64_t>(want, c_tiles);
    *tiles_per_chunk = (int)((c_tiles + chunks - 1) / chunks);
    return (int)((c_tiles + *tiles_per_chunk - 1) / *tiles_per_chunk);
}

// launch geometry of the XCD-aware item order (tile_grid_item): 8 * per blocks, XCD c = items [c * per, (c + 1) * per)
TileGrid make_tile_grid(unsigned nx, unsigned ny) {
    static const bool on = [] { const char *e = getenv("OEA_XCD_MAP"); return !(e && e[0] == '0'); }();
    TileGrid g;
    g.nx = nx; g.ny = ny;
    g.per = on ? (nx * ny + 7u) / 8u : 0u;
    return g;
}
unsigned tile_grid_blocks(const TileGrid &g) { return g.per ? 8u * g.per : g.nx * g.ny; }

// the slot's buffer for an [n, dim] operand (grown if needed, ordered behind its previous use), without the pack launch
int reserve_operand(int slot, int64_t n, int dim, hipStream_t st, PackedOp *out, int64_t *n_pad_out) {
    PackSlot &sl = g_slot[slot];
    const int64_t n_pad = (n + TILE - 1) / TILE * TILE;
    *n_pad_out = n_pad;
    out->kp = (dim + BK - 1) / BK * BK;
    // (+ two tiles of rows: the 256- / 192-candidate tiles of the big pipelines read up to 191 rows past n_pad; products discarded)
    const size_t need = sizeof(float) * (size_t)(n_pad + 2 * TILE) * out->kp;
    if (!sl.used) OEA_CHECK_HIP(hipEventCreateWithFlags(&sl.used, hipEventDisableTiming));
    if (need > sl.cap) {
        if (sl.p) OEA_CHECK_HIP(hipFree(sl.p));
        sl.p = nullptr;
        sl.cap = 0;
        const size_t cap = std::max<size_t>(need + need / 4, (size_t)64 << 20);   // 64 MB = 131,072 rows of K = 128: growth is rare
        OEA_CHECK_HIP(hipMalloc(reinterpret_cast<void **>(&sl.p), cap));
        sl.cap = cap;
    } else if (sl.last != st) {
        OEA_CHECK_HIP(hipStreamWaitEvent(st, sl.used, 0));
    }
    sl.last = st;
    out->p = sl.p;
    return OEA_OK;
}

int pack_operand(int slot, const float *src, int64_t n, int ld, int dim, hipStream_t st, PackedOp *out) {
    int64_t n_pad = 0;
    const int rc = reserve_operand(slot, n, dim, st, out, &n_pad);
    if (rc != OEA_OK) return rc;
    const int64_t total = n_pad * (out->kp / 4);
    pack_rows_kernel<<<(unsigned)std::min<int64_t>(oea::ceil_div(total, 256), 16384), 256, 0, st>>>(src, n, ld, dim, out->p, n_pad,
                                                                                                   out->kp);
    return OEA_OK;
}

int pack_operand_bf16(int slot, const float *src, int64_t n, int ld, int dim, hipStream_t st, PackedOp *out) {
    int64_t n_pad = 0;
    const int rc = reserve_operand(slot, n, dim, st, out, &n_pad);
    if (rc != OEA_OK) return rc;
    const int64_t total = n_pad * (out->kp / 4);
    pack_rows_bf16_kernel<<<(unsigned)std::min<int64_t>(oea::ceil_div(total, 256), 16384), 256, 0, st>>>(
        src, n, ld, dim, reinterpret_cast<uint4 *>(out->p), n_pad, out->kp);
    return OEA_OK;
}

// after the kernels that read the packed operands have been enqueued
int release_packed(hipStream_t st) {
    for (int i = 0; i < 6; ++i)
        if (g_slot[i].used && g_slot[i].last == st) OEA_CHECK_HIP(hipEventRecord(g_slot[i].used, st));
    return OEA_OK;
}

float bf16_eps_rel(int dim, bool k_blocks) {
    const int kp16 = (dim + 15) / 16 * 16;
    // (1) split residue: 3.02 * 2^-18 of |a||b|;
    // (2) fp32 accumulation of the products, bounded term by term with a chopping unit roundoff 2^-23 (the MFMA's internal order
    //     and rounding are not documented): the 3 * min(Kp, 128) products of ONE 128-k block (tile_pipeline_bf16 restarts the
    //     accumulators per block from 5 chunks on; the B-in-registers form only exists for Kp <= 128 = one block) + one rounding
    //     per block sum added;
    // (3) the exact chain's own roundings: fmaf rounds to nearest, <= 2^-24 of a partial sum <= |a||b| per step
    // k_blocks = false (the neighbour sweeps: tile_pipeline_bf16<false>): one accumulation chain over all 3 * Kp products
    const int blocks = k_blocks ? (kp16 + 127) / 128 : 1;
    const int n_acc = blocks > 1 ? 3 * 128 + blocks : 3 * kp16;
    return 1.02f * (3.02f * 3.814697265625e-06f + (float)n_acc * 1.1920928955078125e-07f + (float)(dim + 8) * 5.9604644775390625e-08f);
}

void sim_inner_store_packed(const float *e1p, int64_t n1, const float *e2p, int64_t n2, int kp, int dim, float *out, int64_t ld_out,
                            hipStream_t st, const int32_t *gate) {
    sim_inner_store_kernel<<<dim3((unsigned)ceil_div(n2, TILE), (unsigned)ceil_div(n1, TILE)), 256, 0, st>>>(
        e1p, n1, kp, e2p, n2, kp, dim, out, ld_out, gate);
}

// sample strips on the bf16 split (the neighbour search's since round 6, the CSLS means' since round 5): a threshold is an ESTIMATE
// of where the k-th value lies -- the lists are cut below it by the bound and a row whose list comes out short or long takes the
// exact fallback either way
int sample_strip_bf16_pack(const float *q, int64_t nq, int ldq, const float *c, int64_t n_sample, int ld_sample, int dim, hipStream_t st,
                           const float **qs, const float **ss, int *kp) {
    PackedOp pq, ps;
    int rc = pack_operand_bf16(3, q, nq, ldq, dim, st, &pq);
    if (rc == OEA_OK) rc = pack_operand_bf16(2, c, n_sample, ld_sample, dim, st, &ps);
    if (rc != OEA_OK) return rc;
    *qs = pq.p; *ss = ps.p; *kp = pq.kp;
    return OEA_OK;
}
void sample_strip_bf16_launch(const float *qs, int64_t rows, const float *ss, int64_t n_sample, int kp, int dim, float *strip, hipStream_t st) {
    sim_bf16_store_kernel<<<dim3((unsigned)ceil_div(n_sample, TILE), (unsigned)ceil_div(rows, TILE)), 256, 0, st>>>(qs, rows, kp, ss, n_sample, dim,
                                                                                                                   strip, n_sample);
}

void bf16_tol_bound(const float *a, int64_t na, int lda, const float *b, int64_t nb, int ldb, int dim, bool k_blocks, float *tol_dev,
                    hipStream_t st) {
    unsigned *nmax = reinterpret_cast<unsigned *>(tol_dev);
    row_norm_max_kernel<<<(unsigned)ceil_div(na, 256), 256, 0, st>>>(a, na, lda, dim, nmax + 1);
    if (b) {
        row_norm_max_kernel<<<(unsigned)ceil_div(nb, 256), 256, 0, st>>>(b, nb, ldb, dim, nmax + 2);
        csls_tol_kernel<<<1, 1, 0, st>>>(tol_dev, bf16_eps_rel(dim, k_blocks));
    } else {
        knn_tol_kernel<<<1, 1, 0, st>>>(tol_dev, bf16_eps_rel(dim, k_blocks));
    }
}

}  // namespace oea

extern "C" {

size_t oea_rank_workspace_bytes(int64_t n1) {
    return (size_t)n1 * (sizeof(float) + sizeof(unsigned long long)) + 256;
}

int oea_rank_eval(const float *e1, int64_t n1, int32_t ld1, const float *e2, int64_t n2, int32_t ld2,
                  int32_t dim, int32_t metric, const float *csls_r, const float *csls_c, int64_t gold_offset,
                  int32_t *rank, int32_t *argmax, void *workspace, void *stream) {
    OEA_REQUIRE(e1 && e2 && rank && argmax && workspace, "null pointer");
    OEA_REQUIRE(n1 >= 0 && gold_offset >= 0 && n1 + gold_offset <= n2, "gold of row i is column gold_offset + i <= n2");
    OEA_REQUIRE(ld1 % 4 == 0 && ld2 % 4 == 0 && dim > 0 && dim <= ld1 && dim <= ld2, "ld % 4 == 0, dim <= ld");
    OEA_REQUIRE((csls_r == nullptr) == (csls_c == nullptr), "csls_r and csls_c go together");
    OEA_REQUIRE(n2 < 0x7fffffff, "n2 < 2^31");
    if (n1 == 0) return OEA_OK;
    hipStream_t st = oea::as_stream(stream);
    unsigned long long *keys = static_cast<unsigned long long *>(workspace);
    float *gold = reinterpret_cast<float *>(keys + n1);
    OEA_CHECK_HIP(hipMemsetAsync(keys, 0, sizeof(unsigned long long) * (size_t)n1, st));
    OEA_CHECK_HIP(hipMemsetAsync(rank, 0, sizeof(int32_t) * (size_t)n1, st));
    const unsigned gb = (unsigned)oea::ceil_div(n1, 256);
    int tpc = 1;
    if (metric == OEA_METRIC_INNER) {
        gold_inner_kernel<<<(unsigned)oea::ceil_div(n1, 64), 64, 0, st>>>(e1, n1, ld1, e2 + gold_offset * ld2, ld2, dim, csls_r,
                                                                          csls_c ? csls_c + gold_offset : nullptr, gold);
        const int64_t qt = oea::ceil_div(n1, TILE), ctiles = oea::ceil_div(n2, TILE);
        const int chunks = pick_chunks(qt, ctiles, &tpc);
        const dim3 grid((unsigned)qt, (unsigned)chunks);
        PackedOp p1, p2;
        int rc = pack_operand(0, e1, n1, ld1, dim, st, &p1);
        if (rc == OEA_OK) rc = pack_operand(1, e2, n2, ld2, dim, st, &p2);
        if (rc != OEA_OK) return rc;
        if (csls_r)
            rank_inner_kernel<true><<<grid, 256, 0, st>>>(p1.p, n1, p1.kp, p2.p, n2, p2.kp, dim, gold, csls_r, csls_c, tpc, gold_offset,
                                                          rank, keys, EvalTail{});
        else
            rank_inner_kernel<false><<<grid, 256, 0, st>>>(p1.p, n1, p1.kp, p2.p, n2, p2.kp, dim, gold, csls_r, csls_c, tpc, gold_offset,
                                                           rank, keys, EvalTail{});
        rc = release_packed(st);
        if (rc != OEA_OK) return rc;
    } else if (metric == OEA_METRIC_MANHATTAN || metric == OEA_METRIC_EUCLIDEAN) {
        const int64_t qt = oea::ceil_div(n1, VT), ctiles = oea::ceil_div(n2, VT);
        const int chunks = pick_chunks(qt, ctiles, &tpc);
        if (metric == OEA_METRIC_MANHATTAN) {
            gold_valu_kernel<OEA_METRIC_MANHATTAN><<<gb, 256, 0, st>>>(e1, n1, ld1, e2 + gold_offset * ld2, ld2, dim, csls_r, csls_c ? csls_c + gold_offset : nullptr, gold);
            rank_valu_kernel<OEA_METRIC_MANHATTAN><<<dim3((unsigned)qt, (unsigned)chunks), 256, 0, st>>>(
                e1, n1, ld1, e2, n2, ld2, dim, gold, csls_r, csls_c, tpc, gold_offset, rank, keys);
        } else {
            gold_valu_kernel<OEA_METRIC_EUCLIDEAN><<<gb, 256, 0, st>>>(e1, n1, ld1, e2 + gold_offset * ld2, ld2, dim, csls_r, csls_c ? csls_c + gold_offset : nullptr, gold);
            rank_valu_kernel<OEA_METRIC_EUCLIDEAN><<<dim3((unsigned)qt, (unsigned)chunks), 256, 0, st>>>(
                e1, n1, ld1, e2, n2, ld2, dim, gold, csls_r, csls_c, tpc, gold_offset, rank, keys);
        }
    } else {
        oea::set_error("unknown metric %d", metric);
        return OEA_EINVAL;
    }
    rank_finalize_kernel<<<gb, 256, 0, st>>>(keys, n1, argmax);
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

// ---- inner-product evaluation through the certified bf16 prefilter (see rank_bf16_kernel) --------------------------------------
// record slots: the band around the gold value grows with the tolerance, i.e. with dim (measured on rows whose gold has a
// random rank: 30 records per row at dim 100, 114 at dim 300)
static unsigned bf16_rec_cap(int64_t n1, int dim) { return (unsigned)std::min<int64_t>((96 + (int64_t)dim) * n1 + (1 << 20), (int64_t)1 << 30); }
// an upper bound of the sweep's wave count: pick_chunks gives at most target / q_tiles + 1 chunks per query tile
static int64_t bf16_max_waves(int64_t n1) { return 8 * (oea::ceil_div(n1, TILE) + 16384); }

size_t oea_rank_eval_bf16_workspace_bytes(int64_t n1, int32_t dim) {
    auto a256 = [](size_t x) { return (x + 255) / 256 * 256; };
    return a256(8 * (size_t)n1) + 2 * a256(4 * (size_t)n1) + 256 + a256(4 * (size_t)(2 + bf16_max_waves(n1))) + 8 * (size_t)bf16_rec_cap(n1, dim);
}


constexpr int kBf16WarmTiles = 16;          // the warm-up pass sees 2,048 candidates

// prologue | init | warm-up | sweep | fix-up | finish: six launches; metrics_out (may be NULL) = int64 [nk + 4] on the device
static int rank_eval_bf16_impl(const float *e1, int64_t n1, int32_t ld1, const float *e2, int64_t n2, int32_t ld2, int32_t dim,
                               const float *csls_r, const float *csls_c, int64_t gold_offset, const int32_t *top_k_host, int32_t nk,
                               int32_t *rank, int32_t *argmax, long long *metrics_out, int32_t *status, void *workspace, hipStream_t st) {
    auto a256 = [](size_t x) { return (x + 255) / 256 * 256; };
    char *w = static_cast<char *>(workspace);
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(w);
    float *gold = reinterpret_cast<float *>(w + a256(8 * (size_t)n1));
    unsigned *lbrow = reinterpret_cast<unsigned *>(w + a256(8 * (size_t)n1) + a256(4 * (size_t)n1));
    char *sc = w + a256(8 * (size_t)n1) + 2 * a256(4 * (size_t)n1);
    unsigned *nmax = reinterpret_cast<unsigned *>(sc);              // [2]: max row norms of e1 / e2 (float bits)
    float *tol = reinterpret_cast<float *>(sc + 16);
    long long *fin = reinterpret_cast<long long *>(sc + 64);        // [nk + 4] when the caller wants no metrics
    unsigned *rec_cnt = reinterpret_cast<unsigned *>(sc + 256);     // [0] records, [1] overflow flag, [2 + w] length of wave w's slice
    uint2 *rec = reinterpret_cast<uint2 *>(sc + 256 + a256(4 * (size_t)(2 + bf16_max_waves(n1))));
    const unsigned cap = bf16_rec_cap(n1, dim);
    OEA_CHECK_HIP(hipMemsetAsync(sc, 0, 64, st));                   // norms, tolerance
    PackedOp p1, p2;
    int64_t n1_pad = 0, n2_pad = 0;
    // CSLS means: the rows are packed with two more coordinates (see the prologue) when that costs no k chunk, and the sweep is
    // the plain one.  Its bound: split + accumulation over dim + 2 coordinates on the augmented norms, + the roundings of the
    // exact expression fl(fl(2 s - r) - c) it is compared with (<= 2 * 2^-24 * (2 |s| + |r| + |c|) <= 3.6e-7 * |q'|max |c'|max,
    // the chain's own error inside eps(dim + 2)); OEA_CSLS_AUG=0: the CSLS terms in the sweep's epilogue
    static const bool aug_on = [] { const char *e = getenv("OEA_CSLS_AUG"); return !(e && e[0] == '0'); }();
    const bool aug = csls_r && aug_on && (dim + 2 + BK - 1) / BK == (dim + BK - 1) / BK;
    const int dim_p = aug ? dim + 2 : dim;
    const float *sweep_r = aug ? nullptr : csls_r, *sweep_c = aug ? nullptr : csls_c;
    int rc = reserve_operand(0, n1, dim_p, st, &p1, &n1_pad);
    if (rc == OEA_OK) rc = reserve_operand(1, n2, dim_p, st, &p2, &n2_pad);
    if (rc != OEA_OK) return rc;
    const int64_t items = (n1_pad + n2_pad) * (p1.kp / 4) + 17 * (n1 + n2) + 256;
    rank_bf16_prologue_kernel<<<(unsigned)std::min<int64_t>(oea::ceil_div(items, 256), 16384), 256, 0, st>>>(
        e1, n1, ld1, e2, n2, ld2, dim, gold_offset, reinterpret_cast<uint4 *>(p1.p), n1_pad, reinterpret_cast<uint4 *>(p2.p), n2_pad,
        p1.kp, gold, nmax, rank, csls_r, csls_c, aug ? 1 : 0);
    const unsigned gb = (unsigned)oea::ceil_div(n1, 256);
    rank_bf16_init_kernel<<<gb, 256, 0, st>>>(gold, n1, gold_offset, nmax, aug ? bf16_eps_rel(dim_p, true) + 1.0e-6f : bf16_eps_rel(dim, true), sweep_r, tol,
                                              rank, keys, lbrow, rec_cnt);
    int tpc = 1;
    const int64_t qt = oea::ceil_div(n1, TILE), ctiles = oea::ceil_div(n2, TILE);
    // Kp > 128: 256-candidate tiles, 512 threads, three-stage ring (tile_pipeline_bf16_big); OEA_BF16_BIG=0: the 128 x 128 kernel
    static const bool big_on = [] { const char *e = getenv("OEA_BF16_BIG"); return !(e && e[0] == '0'); }();
    const bool big = big_on && p1.kp > 128;
    const int nw = big ? 8 : 4;
    const int chunks = pick_chunks(qt, big ? oea::ceil_div(n2, BIG_MT) : ctiles, &tpc);
    const int64_t n_waves = (int64_t)nw * qt * chunks;
    const unsigned slice_cap = (unsigned)(cap / std::max<int64_t>(n_waves, 1));
    if (n_waves > bf16_max_waves(n1) || slice_cap < 32) {
        // more workgroups than the workspace was sized for (OEA_RANK_WGS raised) or record slices too small: reported like a record
        // overflow -- the caller takes the fp32 entry point (this used to be a hard error)
        rc = release_packed(st);
        if (rc != OEA_OK) return rc;
        if (status) OEA_CHECK_HIP(hipMemsetAsync(status, 1, 2 * sizeof(int32_t), st));
        if (metrics_out) OEA_CHECK_HIP(hipMemsetAsync(metrics_out, 1, sizeof(long long) * (size_t)(nk + 4), st));
        return OEA_OK;
    }
    // warm-up over 1/16 of the candidate tiles (at most 16 = 2,048 candidates, 3 % of a 70,000-row sweep); a small candidate
    // set needs none: every workgroup sees most of it anyway
    const int warm = (int)std::min<int64_t>(kBf16WarmTiles, ctiles / 16);
    const TileGrid gw = make_tile_grid((unsigned)qt, 1), gs = make_tile_grid((unsigned)qt, (unsigned)chunks);
    // Kp <= 128 (dim <= 128): the candidates' operand stays in registers (OEA_BF16_BREG=0: both operands through LDS)
    static const bool breg_on = [] { const char *e = getenv("OEA_BF16_BREG"); return !(e && e[0] == '0'); }();
    // (with the CSLS terms the epilogue's registers + 32 NCH of B spill from NCH = 3 on: 6.5 -> 7.6 ms, stays on the LDS pipeline)
    const int nch = (breg_on && p1.kp <= (sweep_r ? 64 : 128)) ? p1.kp / 32 : 0;
#define OEA_BF16_LAUNCH(K, GRID, TPC) K<<<tile_grid_blocks(GRID), 256, 0, st>>>(p1.p, n1, p1.kp, p2.p, n2, dim_p, gold, tol, sweep_r, sweep_c, TPC, \
                                                                                gold_offset, rank, lbrow, rec, rec_cnt, slice_cap, GRID)
#define OEA_BF16_SWEEP(W, C, GRID, TPC)                                                                 \
    do {                                                                                                \
        if (nch == 4) OEA_BF16_LAUNCH((rank_bf16_breg_kernel<W, C, 4>), GRID, TPC);                     \
        else if (nch == 3) OEA_BF16_LAUNCH((rank_bf16_breg_kernel<W, C, 3>), GRID, TPC);                \
        else if (nch == 2) OEA_BF16_LAUNCH((rank_bf16_breg_kernel<W, C, 2>), GRID, TPC);                \
        else if (nch == 1) OEA_BF16_LAUNCH((rank_bf16_breg_kernel<W, C, 1>), GRID, TPC);                \
        else OEA_BF16_LAUNCH((rank_bf16_kernel<W, C>), GRID, TPC);                                      \
    } while (0)
#define OEA_BF16_BIG_SWEEP(C, PF)                                                                                                    \
    do {                                                                                                                            \
        /* the attribute belongs to (function, DEVICE): set on every call (cheap), not once per process */             \
        OEA_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(rank_bf16_big_kernel<C, PF>), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                          BIG_LDS_BYTES));                                                                          \
        rank_bf16_big_kernel<C, PF><<<tile_grid_blocks(gs), 512, BIG_LDS_BYTES, st>>>(p1.p, n1, p1.kp, p2.p, n2, dim_p, gold, tol, sweep_r, sweep_c, tpc, \
                                                                                     gold_offset, rank, lbrow, rec, rec_cnt, slice_cap, gs);    \
        OEA_CHECK_HIP(hipGetLastError());                                                                                           \
    } while (0)
    if (sweep_r) {
        if (warm >= 2) OEA_BF16_SWEEP(true, true, gw, warm);
        if (big) OEA_BF16_BIG_SWEEP(true, false);      // (CSLS terms in the epilogue -- only when the two extra coordinates would cost a
        else OEA_BF16_SWEEP(false, true, gs, tpc);     //  chunk: the prefetched forms spill there)
    } else {
        if (warm >= 2) OEA_BF16_SWEEP(true, false, gw, warm);
        if (big) OEA_BF16_BIG_SWEEP(false, true);
        else OEA_BF16_SWEEP(false, false, gs, tpc);
    }
#undef OEA_BF16_BIG_SWEEP
#undef OEA_BF16_SWEEP
#undef OEA_BF16_LAUNCH
    rc = release_packed(st);
    if (rc != OEA_OK) return rc;
    rank_bf16_fixup_kernel<<<(unsigned)std::min<int64_t>(oea::ceil_div(n_waves, 4), 2048), 256, 0, st>>>(
        e1, ld1, e2, ld2, dim, gold, gold_offset, csls_r, csls_c, rec, rec_cnt, (unsigned)n_waves, slice_cap, rank, keys);
    int t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < nk; ++i) t[i] = top_k_host[i];
    long long *out = metrics_out ? metrics_out : fin;
    rank_bf16_finish_kernel<<<1, 1024, 0, st>>>(rank, keys, n1, make_int4(t[0], t[1], t[2], t[3]), make_int4(t[4], t[5], t[6], t[7]), nk,
                                                argmax, out, rec_cnt);
    if (status) {
        OEA_CHECK_HIP(hipMemcpyAsync(status, rec_cnt + 1, sizeof(int32_t), hipMemcpyDeviceToDevice, st));
        OEA_CHECK_HIP(hipMemcpyAsync(status + 1, rec_cnt, sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    }
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

int oea_rank_eval_bf16(const float *e1, int64_t n1, int32_t ld1, const float *e2, int64_t n2, int32_t ld2, int32_t dim,
                       int64_t gold_offset, int32_t *rank, int32_t *argmax, int32_t *status, void *workspace, void *stream) {
    OEA_REQUIRE(e1 && e2 && rank && argmax && status && workspace, "null pointer");
    OEA_REQUIRE(n1 >= 0 && gold_offset >= 0 && n1 + gold_offset <= n2, "gold of row i is column gold_offset + i <= n2");
    OEA_REQUIRE(ld1 % 4 == 0 && ld2 % 4 == 0 && dim > 0 && dim <= ld1 && dim <= ld2, "ld % 4 == 0, dim <= ld");
    OEA_REQUIRE(n2 < 0x7fffffff && n1 < 0x7fffffff, "n < 2^31");
    hipStream_t st = oea::as_stream(stream);
    if (n1 == 0) { OEA_CHECK_HIP(hipMemsetAsync(status, 0, 2 * sizeof(int32_t), st)); return OEA_OK; }
    return rank_eval_bf16_impl(e1, n1, ld1, e2, n2, ld2, dim, nullptr, nullptr, gold_offset, nullptr, 0, rank, argmax, nullptr, status,
                               workspace, st);
}

int oea_rank_eval_bf16_csls(const float *e1, int64_t n1, int32_t ld1, const float *e2, int64_t n2, int32_t ld2, int32_t dim,
                            const float *csls_r, const float *csls_c, int64_t gold_offset, int32_t *rank, int32_t *argmax, int32_t *status,
                            void *workspace, void *stream) {
    OEA_REQUIRE(e1 && e2 && rank && argmax && status && workspace, "null pointer");
    OEA_REQUIRE((csls_r == nullptr) == (csls_c == nullptr), "csls_r and csls_c: both or neither");
    OEA_REQUIRE(n1 >= 0 && gold_offset >= 0 && n1 + gold_offset <= n2, "gold of row i is column gold_offset + i <= n2");
    OEA_REQUIRE(ld1 % 4 == 0 && ld2 % 4 == 0 && dim > 0 && dim <= ld1 && dim <= ld2, "ld % 4 == 0, dim <= ld");
    OEA_REQUIRE(n2 < 0x7fffffff && n1 < 0x7fffffff, "n < 2^31");
    hipStream_t st = oea::as_stream(stream);
    if (n1 == 0) { OEA_CHECK_HIP(hipMemsetAsync(status, 0, 2 * sizeof(int32_t), st)); return OEA_OK; }
    return rank_eval_bf16_impl(e1, n1, ld1, e2, n2, ld2, dim, csls_r, csls_c, gold_offset, nullptr, 0, rank, argmax, nullptr, status,
                               workspace, st);
}

int oea_rank_eval_metrics_bf16(const float *e1, int64_t n1, int32_t ld1, const float *e2, int64_t n2, int32_t ld2, int32_t dim,
                               const float *csls_r, const float *csls_c, int64_t gold_offset, const int32_t *top_k_host, int32_t nk,
                               int32_t *rank, int32_t *argmax, int64_t *out_dev, void *workspace, void *stream) {
    OEA_REQUIRE(e1 && e2 && rank && argmax && workspace && top_k_host && out_dev, "null pointer");
    OEA_REQUIRE((csls_r == nullptr) == (csls_c == nullptr), "csls_r and csls_c go together");
    OEA_REQUIRE(n1 > 0 && gold_offset >= 0 && n1 + gold_offset <= n2, "gold of row i is column gold_offset + i <= n2");
    OEA_REQUIRE(ld1 % 4 == 0 && ld2 % 4 == 0 && dim > 0 && dim <= ld1 && dim <= ld2, "ld % 4 == 0, dim <= ld");
    OEA_REQUIRE(n2 < 0x7fffffff && n1 < 0x7fffffff && nk >= 1 && nk <= 8, "n < 2^31, 1 <= len(top_k) <= 8");
    return rank_eval_bf16_impl(e1, n1, ld1, e2, n2, ld2, dim, csls_r, csls_c, gold_offset, top_k_host, nk, rank, argmax,
                               reinterpret_cast<long long *>(out_dev), nullptr, workspace, oea::as_stream(stream));
}

int oea_sim_bf16_matrix(const float *e1, int64_t n1, int32_t ld1, const float *e2, int64_t n2, int32_t ld2, int32_t dim, float *out,
                        int64_t ld_out, void *stream) {
    OEA_REQUIRE(e1 && e2 && out && ld_out >= n2 && dim > 0 && dim <= ld1 && dim <= ld2 && ld1 % 4 == 0 && ld2 % 4 == 0, "arguments");
    if (n1 == 0 || n2 == 0) return OEA_OK;
    hipStream_t st = oea::as_stream(stream);
    PackedOp p1, p2;
    int rc = pack_operand_bf16(0, e1, n1, ld1, dim, st, &p1);
    if (rc == OEA_OK) rc = pack_operand_bf16(1, e2, n2, ld2, dim, st, &p2);
    if (rc != OEA_OK) return rc;
    sim_bf16_store_kernel<<<dim3((unsigned)oea::ceil_div(n2, TILE), (unsigned)oea::ceil_div(n1, TILE)), 256, 0, st>>>(p1.p, n1, p1.kp, p2.p,
                                                                                                                     n2, dim, out, ld_out);
    rc = release_packed(st);
    if (rc != OEA_OK) return rc;
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

int oea_rank_metrics(const int32_t *rank, int64_t n, const int32_t *top_k_host, int32_t nk, int64_t *hits_dev,
                     int64_t *rank_sum_dev, double *rr_sum_dev, void *stream) {
    OEA_REQUIRE(rank && top_k_host && hits_dev && rank_sum_dev && rr_sum_dev, "null pointer");
    OEA_REQUIRE(nk >= 1 && nk <= 8, "1 <= len(top_k) <= 8");
    int t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < nk; ++i) t[i] = top_k_host[i];
    rank_metrics_kernel<<<1, 1024, 0, oea::as_stream(stream)>>>(rank, n, make_int4(t[0], t[1], t[2], t[3]),
                                                               make_int4(t[4], t[5], t[6], t[7]), nk,
                                                               (long long *)hits_dev, (long long *)rank_sum_dev, rr_sum_dev);
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

size_t oea_rank_eval_metrics_workspace_bytes(int64_t n1) {
    const size_t tiles = (size_t)((n1 + TILE - 1) / TILE);
    return oea_rank_workspace_bytes(n1) + 256 + tiles * (10 * sizeof(long long) + sizeof(unsigned)) + 64;
}

int oea_rank_eval_metrics(const float *e1, int64_t n1, int32_t ld1, const float *e2, int64_t n2, int32_t ld2, int32_t dim,
                          const float *csls_r, const float *csls_c, int64_t gold_offset, const int32_t *top_k_host, int32_t nk,
                          int32_t *rank, int32_t *argmax, int64_t *hits_and_rank_sum_dev, double *rr_sum_dev, void *workspace,
                          void *stream) {
    OEA_REQUIRE(e1 && e2 && rank && argmax && workspace && top_k_host && hits_and_rank_sum_dev && rr_sum_dev, "null pointer");
    OEA_REQUIRE(n1 > 0 && gold_offset >= 0 && n1 + gold_offset <= n2, "gold of row i is column gold_offset + i <= n2");
    OEA_REQUIRE(ld1 % 4 == 0 && ld2 % 4 == 0 && dim > 0 && dim <= ld1 && dim <= ld2, "ld % 4 == 0, dim <= ld");
    OEA_REQUIRE((csls_r == nullptr) == (csls_c == nullptr), "csls_r and csls_c go together");
    OEA_REQUIRE(n2 < 0x7fffffff && nk >= 1 && nk <= 8, "n2 < 2^31, 1 <= len(top_k) <= 8");
    hipStream_t st = oea::as_stream(stream);
    unsigned long long *keys = static_cast<unsigned long long *>(workspace);
    float *gold = reinterpret_cast<float *>(keys + n1);
    const int64_t qt = oea::ceil_div(n1, TILE), ctiles = oea::ceil_div(n2, TILE);
    char *extra = reinterpret_cast<char *>(workspace) + ((oea_rank_workspace_bytes(n1) + 15) / 16) * 16;
    long long *tile_part = reinterpret_cast<long long *>(extra);
    unsigned *done = reinterpret_cast<unsigned *>(extra + (size_t)qt * 10 * sizeof(long long));
    PackedOp p1, p2;
    int64_t n1_pad = 0, n2_pad = 0;
    int rc = reserve_operand(0, n1, dim, st, &p1, &n1_pad);
    if (rc == OEA_OK) rc = reserve_operand(1, n2, dim, st, &p2, &n2_pad);
    if (rc != OEA_OK) return rc;
    const int64_t work = (n1_pad + n2_pad) * (p1.kp / 4);
    eval_prologue_kernel<<<(unsigned)std::min<int64_t>(oea::ceil_div(work, 256), 16384), 256, 0, st>>>(
        e1, n1, ld1, e2, n2, ld2, dim, p1.p, n1_pad, p2.p, n2_pad, p1.kp, csls_r, csls_c, gold_offset, gold, keys, rank, done,
        (int)qt + 1);
    EvalTail tail{};
    tail.done = done;
    tail.tile_part = tile_part;
    tail.argmax = argmax;
    tail.hits = reinterpret_cast<long long *>(hits_and_rank_sum_dev);
    tail.rr_sum = rr_sum_dev;
    tail.nk = nk;
    for (int i = 0; i < nk; ++i) tail.tk[i] = top_k_host[i];
    int tpc = 1;
    const int chunks = pick_chunks(qt, ctiles, &tpc);
    const dim3 grid((unsigned)qt, (unsigned)chunks);
    if (csls_r)
        rank_inner_kernel<true><<<grid, 256, 0, st>>>(p1.p, n1, p1.kp, p2.p, n2, p2.kp, dim, gold, csls_r, csls_c, tpc,
                                                      gold_offset, rank, keys, tail);
    else
        rank_inner_kernel<false><<<grid, 256, 0, st>>>(p1.p, n1, p1.kp, p2.p, n2, p2.kp, dim, gold, csls_r, csls_c, tpc,
                                                       gold_offset, rank, keys, tail);
    rc = release_packed(st);
    if (rc != OEA_OK) return rc;
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

int oea_sim_matrix(const float *e1, int64_t n1, int32_t ld1, const float *e2, int64_t n2, int32_t ld2,
                   int32_t dim, int32_t metric, float *out, int64_t ld_out, void *stream) {
    OEA_REQUIRE(e1 && e2 && out, "null pointer");
    OEA_REQUIRE(ld1 % 4 == 0 && ld2 % 4 == 0 && dim > 0 && dim <= ld1 && dim <= ld2 && ld_out >= n2 && ld_out < (1 << 24), "shapes");
    if (n1 == 0 || n2 == 0) return OEA_OK;
    hipStream_t st = oea::as_stream(stream);
    if (metric == OEA_METRIC_INNER) {
        PackedOp p1, p2;
        int rc = pack_operand(0, e1, n1, ld1, dim, st, &p1);
        if (rc == OEA_OK) rc = pack_operand(1, e2, n2, ld2, dim, st, &p2);
        if (rc != OEA_OK) return rc;
        sim_inner_store_packed(p1.p, n1, p2.p, n2, p1.kp, dim, out, ld_out, st);
        rc = release_packed(st);
        if (rc != OEA_OK) return rc;
    } else if (metric == OEA_METRIC_MANHATTAN) {
        sim_valu_store_kernel<OEA_METRIC_MANHATTAN><<<dim3((unsigned)oea::ceil_div(n2, VT), (unsigned)oea::ceil_div(n1, VT)), 256, 0, st>>>(
            e1, n1, ld1, e2, n2, ld2, dim, out, ld_out);
    } else if (metric == OEA_METRIC_EUCLIDEAN) {
        sim_valu_store_kernel<OEA_METRIC_EUCLIDEAN><<<dim3((unsigned)oea::ceil_div(n2, VT), (unsigned)oea::ceil_div(n1, VT)), 256, 0, st>>>(
            e1, n1, ld1, e2, n2, ld2, dim, out, ld_out);
    } else if (metric == OEA_METRIC_MANHATTAN_F32) {
        sim_l1_f32_store_kernel<<<dim3((unsigned)oea::ceil_div(n2, LT), (unsigned)oea::ceil_div(n1, LT)), 256, 0, st>>>(
            e1, n1, ld1, e2, n2, ld2, dim, out, ld_out);
    } else {
        oea::set_error("unknown metric %d", metric);
        return OEA_EINVAL;
    }
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

int oea_rank_rows(const float *s, int64_t n_rows, int64_t nc, int64_t ld, const int32_t *gold_idx, int32_t *rank,
                  int32_t *argmax, void *stream) {
    OEA_REQUIRE(s && gold_idx && rank && argmax, "null pointer");
    OEA_REQUIRE(nc >= 1 && nc < 0x7fffffff && ld >= nc && n_rows < 0x7fffffff, "1 <= nc <= ld");
    if (n_rows == 0) return OEA_OK;
    rank_rows_kernel<<<(unsigned)n_rows, 256, 0, oea::as_stream(stream)>>>(s, nc, ld, gold_idx, rank, argmax);
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

}  // extern "C"
