// transr_step.hip -- TransR's training step (models/trans/transr.py:13-50 of the reference), grouped by relation.
//
//   x = l2_normalize(ent)[e],  y = M_r x  (M_r = rel_matrix[r] as d x d, row-major),  y' = l2_normalize(y),
//   loss = sum_i relu(margin + |h'+r-t'|^2 - |nh'+nr-nt'|^2),  r = l2_normalize(rel)[r] (not projected),
// one Adagrad (or SGD) over ent_embeds, rel_embeds and rel_matrix; rel_matrix gets TF's IndexedSlices update (duplicate
// relations summed, relations absent from the batch untouched).
//
// The reference gathers one d x d matrix per projected row (800 MB per step at d = 100, batch 5,000).  Here a projection
// ITEM is a (pair, side) couple -- side 0 / 1 / 2 / 3 = h / t of the positive, h / t of the negative, each with its own
// triple's relation -- and the items are counting-sorted by relation (stable: item order inside a relation), then cut into
// tiles of at most T items of one relation.  Per step:
//   rank      per block of 256 items: rank of an item among the earlier items of the block with the same relation
//             + the block's relation histogram
//   scan      one workgroup: per-(block, relation) offsets, relation offsets, tiles per relation, the tile table
//   scatter   sorted[offset + rank] = item
//   fwd       one workgroup per tile: M_r and the tile's normalised entity rows in LDS, Y = X M_r^T on
//             v_mfma_f32_16x16x4_f32 (exact fp32), y' and 1/|y| per item
//   loss      one wave per pair: hinge, dL/dr into the step's relation scratch, dy = (g - y'(y'.g)) / |y| per item
//   bwd       one workgroup per tile: dX = dY M_r into the step's entity scratch, dM = dY^T X; a relation with one tile
//             applies the optimiser to its matrix right there, the tiles of a larger relation write per-tile slabs
//   mapply    relations with more than one tile: their slabs summed in tile order (no atomics: the same bits run to
//             run), then the optimiser
// The entity / relation rows are finished by the step engine's apply phase (oea_triple_step_phase, OEA_PHASE_APPLY).
#include "common.h"

#include <algorithm>

namespace {

using oea::flag_t;
using oea::grad_t;

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int T = 64;            // items per tile
constexpr int SB = 256;          // items per block of the sort
constexpr int kMaxDim = 128;

struct TrWs {
    int32_t *hist;       // [nb][n_rel]: block histogram, then the block's offset per relation
    int32_t *rank;       // [N]
    int32_t *sorted;     // [N]
    int32_t *rel_tile0;  // [n_rel]
    int32_t *rel_ntiles; // [n_rel]
    int32_t *n_tiles;    // [1]
    int4 *tiles;         // [max_tiles]: (relation, first sorted position, count, 0)
    float *yp;           // [N][dp]: y'
    float *inv;          // [N]: 1 / |y|
    float *dy;           // [N][dp]: dL/dy
    float *slab;         // [max_tiles][d * d]: per-tile dM of relations with more than one tile
};

static int dpad(int dim) { return (dim + 15) / 16 * 16; }
static int64_t max_tiles(int64_t n_items, int64_t n_rel) { return oea::ceil_div(n_items, T) + n_rel; }

static size_t tr_layout(int64_t n_rel, int32_t dim, int64_t n_pos, void *base, TrWs *ws) {
    const int64_t N = 4 * n_pos, nb = oea::ceil_div(N, SB), mt = max_tiles(N, n_rel), dp = dpad(dim);
    size_t off = 0;
    char *b = static_cast<char *>(base);
    auto take = [&](size_t bytes) { size_t o = off; off += oea::align256(bytes); return b ? b + o : nullptr; };
    TrWs w;
    w.hist = (int32_t *)take(sizeof(int32_t) * (size_t)(nb * n_rel));
    w.rank = (int32_t *)take(sizeof(int32_t) * (size_t)N);
    w.sorted = (int32_t *)take(sizeof(int32_t) * (size_t)N);
    w.rel_tile0 = (int32_t *)take(sizeof(int32_t) * (size_t)n_rel);
    w.rel_ntiles = (int32_t *)take(sizeof(int32_t) * (size_t)n_rel);
    w.n_tiles = (int32_t *)take(sizeof(int32_t));
    w.tiles = (int4 *)take(sizeof(int4) * (size_t)mt);
    w.yp = (float *)take(sizeof(float) * (size_t)(N * dp));
    w.inv = (float *)take(sizeof(float) * (size_t)N);
    w.dy = (float *)take(sizeof(float) * (size_t)(N * dp));
    w.slab = (float *)take(sizeof(float) * (size_t)(mt * (int64_t)dim * dim));
    if (ws) *ws = w;
    return off;
}

// item i = 4 p + side: side 0 / 1 = head / tail of pos p, 2 / 3 = head / tail of neg p
__device__ __forceinline__ const int32_t *item_triple(const int32_t *pos, const int32_t *neg, int32_t i) {
    return ((i & 3) < 2 ? pos : neg) + 3 * (int64_t)(i >> 2);
}
__device__ __forceinline__ int32_t item_rel(const int32_t *pos, const int32_t *neg, int32_t i) { return item_triple(pos, neg, i)[1]; }
__device__ __forceinline__ int32_t item_ent(const int32_t *pos, const int32_t *neg, int32_t i) {
    return item_triple(pos, neg, i)[(i & 1) ? 2 : 0];
}

// ---- counting sort by relation (stable) ----------------------------------------------------------------------------------
__global__ __launch_bounds__(SB) void rank_kernel(const int32_t *__restrict__ pos, const int32_t *__restrict__ neg, int64_t N,
                                                  int64_t n_rel, int32_t *__restrict__ hist, int32_t *__restrict__ rank) {
    __shared__ int32_t rs[SB];
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * SB + tid;
    const int32_t r = i < N ? item_rel(pos, neg, (int32_t)i) : -1;
    rs[tid] = r;
    __syncthreads();
    if (i >= N) return;
    int k = 0;
    for (int j = 0; j < tid; ++j) k += rs[j] == r;
    rank[i] = k;
    atomicAdd(&hist[(int64_t)blockIdx.x * n_rel + r], 1);
}

// one workgroup of 1024 threads: relation counts and offsets, tiles per relation, the tile table
__global__ __launch_bounds__(1024) void scan_kernel(int32_t *__restrict__ hist, int64_t nb, int64_t n_rel,
                                                    int32_t *__restrict__ rel_tile0, int32_t *__restrict__ rel_ntiles,
                                                    int32_t *__restrict__ n_tiles, int4 *__restrict__ tiles, int tile) {
    __shared__ int32_t s_cnt[1024], s_nt[1024];
    __shared__ int32_t carry_items, carry_tiles;
    const int tid = threadIdx.x;
    if (tid == 0) { carry_items = 0; carry_tiles = 0; }
    __syncthreads();
    for (int64_t r0 = 0; r0 < n_rel; r0 += 1024) {
        const int64_t r = r0 + tid;
        int32_t c = 0;
        if (r < n_rel)
            for (int64_t b = 0; b < nb; ++b) {           // per-block counts -> offsets inside the relation's segment
                int32_t *h = hist + b * n_rel + r;
                const int32_t v = *h;
                *h = c;
                c += v;
            }
        const int32_t nt = (c + tile - 1) / tile;
        s_cnt[tid] = c;
        s_nt[tid] = nt;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {       // inclusive scans (Hillis-Steele)
            const int32_t a = tid >= off ? s_cnt[tid - off] : 0, t = tid >= off ? s_nt[tid - off] : 0;
            __syncthreads();
            s_cnt[tid] += a;
            s_nt[tid] += t;
            __syncthreads();
        }
        const int32_t item0 = carry_items + s_cnt[tid] - c, tile0 = carry_tiles + s_nt[tid] - nt;
        if (r < n_rel) {
            rel_tile0[r] = tile0;
            rel_ntiles[r] = nt;
            for (int64_t b = 0; b < nb; ++b) hist[b * n_rel + r] += item0;
            for (int32_t k = 0; k < nt; ++k) tiles[tile0 + k] = make_int4((int32_t)r, item0 + k * tile, min(tile, c - k * tile), 0);
        }
        __syncthreads();
        if (tid == 1023) { carry_items += s_cnt[1023]; carry_tiles += s_nt[1023]; }
        __syncthreads();
    }
    if (tid == 0) *n_tiles = carry_tiles;
}

__global__ __launch_bounds__(SB) void scatter_kernel(const int32_t *__restrict__ pos, const int32_t *__restrict__ neg, int64_t N,
                                                     int64_t n_rel, const int32_t *__restrict__ hist,
                                                     const int32_t *__restrict__ rank, int32_t *__restrict__ sorted) {
    const int64_t i = (int64_t)blockIdx.x * SB + threadIdx.x;
    if (i >= N) return;
    const int32_t r = item_rel(pos, neg, (int32_t)i);
    sorted[hist[(int64_t)blockIdx.x * n_rel + r] + rank[i]] = (int32_t)i;
}

// ---- tile staging (LDS row stride S = DP + 4: S / 4 odd, so the 16 rows x 4 columns an MFMA operand read touches fall on 64
// distinct banks) ----------------------------------------------------------------------------------------------------------
template <int DP>
__device__ __forceinline__ void stage_matrix(const float *__restrict__ Mg, int dim, float *Ms) {
    constexpr int S = DP + 4;
    for (int e = threadIdx.x; e < DP * DP; e += blockDim.x) {
        const int j = e / DP, k = e - j * DP;
        Ms[j * S + k] = (j < dim && k < dim) ? Mg[j * dim + k] : 0.f;
    }
}

// the tile's normalised entity rows (rows >= count zero); one wave per row
template <int DP>
__device__ __forceinline__ void stage_rows(const float *__restrict__ ent, int ld, int dim, int l2n, const int32_t *__restrict__ pos,
                                           const int32_t *__restrict__ neg, const int32_t *items, int count, int tile, float *Xs) {
    constexpr int S = DP + 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int i = wave; i < tile; i += nw) {
        float v0 = 0.f, v1 = 0.f;
        if (i < count) {
            const float *row = ent + (int64_t)item_ent(pos, neg, items[i]) * ld;
            if (lane < dim) v0 = row[lane];
            if (lane + 64 < dim) v1 = row[lane + 64];
        }
        const float s = oea::group_sum<64>(v0 * v0 + v1 * v1);
        const float sc = l2n ? rsqrtf(fmaxf(s, 1e-12f)) : 1.f;
        if (lane < DP) Xs[i * S + lane] = v0 * sc;
        if (lane + 64 < DP) Xs[i * S + lane + 64] = v1 * sc;
    }
}

template <int DP>
__global__ __launch_bounds__(256) void fwd_kernel(const float *__restrict__ ent, int ld, int dim, int l2n,
                                                  const float *__restrict__ rel_matrix, const int32_t *__restrict__ pos,
                                                  const int32_t *__restrict__ neg, TrWs ws, int tile) {
    constexpr int S = DP + 4, NCB = DP / 16;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int32_t items[T];
    if ((int)blockIdx.x >= *ws.n_tiles) return;
    const int4 tl = ws.tiles[blockIdx.x];
    const int r = tl.x, first = tl.y, count = tl.z;
    float *Ms = lds, *Xs = lds + DP * S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < T) items[tid] = tid < count ? ws.sorted[first + tid] : 0;
    stage_matrix<DP>(rel_matrix + (int64_t)r * dim * dim, dim, Ms);
    __syncthreads();
    stage_rows<DP>(ent, ld, dim, l2n, pos, neg, items, count, tile, Xs);
    __syncthreads();
    const int i0 = 16 * wave;
    if (i0 < count) {                                  // wave-uniform: wave w owns rows 16 w .. 16 w + 15 of the tile
        f32x4 acc[NCB];
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
        // Y[i][j] = sum_k X[i][k] M[j][k]: A = X (lane: row l & 15, k = l >> 4), B[k][j] = M[j][k]
        const float *ap = Xs + (i0 + (lane & 15)) * S + (lane >> 4);
        const float *bp = Ms + (lane & 15) * S + (lane >> 4);
#pragma unroll 4
        for (int k0 = 0; k0 < DP; k0 += 4) {
            const float a = ap[k0];
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bp[16 * cb * S + k0], acc[cb], 0, 0, 0);
        }
        // row norms straight from the accumulators (D: row 4 (l >> 4) + reg, column 16 cb + (l & 15)): the 16 lanes of a DPP row
        // hold one row's columns.  (Going through LDS instead -- Y over the wave's X rows, then one reduction per row -- gave wrong
        // rows 4k + 1 and 4k + 2 at DP = 128 and right ones at DP <= 112; the cause was not found.)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float ss = 0.f;
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) ss += acc[cb][q] * acc[cb][q];
            ss = oea::group_sum<16>(ss);
            const float inv = rsqrtf(fmaxf(ss, 1e-12f));
            const int i = i0 + 4 * (lane >> 4) + q;
            if (i < count) {
                const int64_t it = items[i];
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) ws.yp[it * DP + 16 * cb + (lane & 15)] = acc[cb][q] * inv;
                if ((lane & 15) == 0) ws.inv[it] = inv;
            }
        }
    }
}

// one wave per (pos p, neg p) pair
template <int DP>
__global__ __launch_bounds__(256) void loss_kernel(const float *__restrict__ rel, int ld, int dim, int rel_l2n,
                                                   const int32_t *__restrict__ pos, const int32_t *__restrict__ neg, int64_t n,
                                                   float margin, TrWs ws, grad_t *__restrict__ rel_grad,
                                                   flag_t *__restrict__ rel_touched, double *__restrict__ loss_accum) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (p >= n) return;
    const int pr = pos[3 * p + 1], nr = neg[3 * p + 1];
    float y[4][2], rp[2], rn[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int c = lane + 64 * h;
#pragma unroll
        for (int s = 0; s < 4; ++s) y[s][h] = c < DP ? ws.yp[(4 * p + s) * DP + c] : 0.f;
        rp[h] = c < dim ? rel[(int64_t)pr * ld + c] : 0.f;
        rn[h] = c < dim ? rel[(int64_t)nr * ld + c] : 0.f;
    }
    if (rel_l2n) {
        const float ip = rsqrtf(fmaxf(oea::group_sum<64>(rp[0] * rp[0] + rp[1] * rp[1]), 1e-12f));
        const float in = rsqrtf(fmaxf(oea::group_sum<64>(rn[0] * rn[0] + rn[1] * rn[1]), 1e-12f));
#pragma unroll
        for (int h = 0; h < 2; ++h) { rp[h] *= ip; rn[h] *= in; }
    }
    float dpv[2], dnv[2], sp = 0.f, sn = 0.f;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        dpv[h] = y[0][h] + rp[h] - y[1][h];
        dnv[h] = y[2][h] + rn[h] - y[3][h];
        sp += dpv[h] * dpv[h];
        sn += dnv[h] * dnv[h];
    }
    sp = oea::group_sum<64>(sp);
    sn = oea::group_sum<64>(sn);
    const float l = margin + sp - sn;
    const bool on = l > 0.f;
    // dL/dy' of the four items: +gp, -gp, -gn, +gn (gp = 2 (h + r - t), gn = 2 (nh + nr - nt))
    float g[4][2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float gp = on ? 2.f * dpv[h] : 0.f, gn = on ? 2.f * dnv[h] : 0.f;
        g[0][h] = gp; g[1][h] = -gp; g[2][h] = -gn; g[3][h] = gn;
        const int c = lane + 64 * h;
        if (on && c < dim) {
            oea::grad_add(rel_grad + (int64_t)pr * ld + c, gp);
            oea::grad_add(rel_grad + (int64_t)nr * ld + c, -gn);
        }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const float dot = oea::group_sum<64>(y[s][0] * g[s][0] + y[s][1] * g[s][1]);
        const float inv = ws.inv[4 * p + s];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int c = lane + 64 * h;
            if (c < DP) ws.dy[(4 * p + s) * DP + c] = (g[s][h] - y[s][h] * dot) * inv;
        }
    }
    if (lane == 0) {
        rel_touched[pr] = 1;
        rel_touched[nr] = 1;
        if (on) atomicAdd(loss_accum, (double)l);
    }
}

__device__ __forceinline__ void matrix_update(float *__restrict__ m, float *__restrict__ acc, float g, float lr, int adagrad) {
    if (adagrad) {
        const float a = *acc + g * g;
        *acc = a;
        *m = *m - lr * g / sqrtf(a);
    } else {
        *m = *m - lr * g;
    }
}

template <int DP>
__global__ __launch_bounds__(256) void bwd_kernel(const float *__restrict__ ent, int ld, int dim, int l2n,
                                                  float *__restrict__ rel_matrix, float *__restrict__ rel_matrix_acc,
                                                  const int32_t *__restrict__ pos, const int32_t *__restrict__ neg, TrWs ws,
                                                  grad_t *__restrict__ ent_grad, flag_t *__restrict__ ent_touched, float lr,
                                                  int adagrad, int tile) {
    constexpr int S = DP + 4, NCB = DP / 16;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int32_t items[T];
    if ((int)blockIdx.x >= *ws.n_tiles) return;
    const int4 tl = ws.tiles[blockIdx.x];
    const int r = tl.x, first = tl.y, count = tl.z;
    // LDS: [M_r, then the tile's X once dX is done | dY]: (max(DP, tile) + tile) x S floats
    float *Ms = lds, *Xs = lds, *Ds = lds + (DP > tile ? DP : tile) * S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t dd = (int64_t)dim * dim;
    if (tid < T) items[tid] = tid < count ? ws.sorted[first + tid] : 0;
    stage_matrix<DP>(rel_matrix + r * dd, dim, Ms);
    __syncthreads();                                   // items[]
    for (int e = tid; e < tile * DP; e += blockDim.x) {
        const int i = e / DP, k = e - i * DP;
        Ds[i * S + k] = i < count ? ws.dy[(int64_t)items[i] * DP + k] : 0.f;
    }
    __syncthreads();
    const int i0 = 16 * wave;
    if (i0 < count) {                                  // dX = dY M: wave w owns rows 16 w .. 16 w + 15
        f32x4 acc[NCB];
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float *ap = Ds + (i0 + (lane & 15)) * S + (lane >> 4);       // A[i][j] = dY[i][j]
        const float *bp = Ms + (lane >> 4) * S + (lane & 15);              // B[j][k] = M[j][k]
#pragma unroll 4
        for (int j0 = 0; j0 < DP; j0 += 4) {
            const float a = ap[j0];
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bp[j0 * S + 16 * cb], acc[cb], 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + 4 * (lane >> 4) + q;
            if (i < count) {
                const int64_t e = item_ent(pos, neg, items[i]);
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) {
                    const int k = 16 * cb + (lane & 15);
                    if (k < dim) oea::grad_add(ent_grad + e * ld + k, acc[cb][q]);
                }
                if ((lane & 15) == 0) ent_touched[e] = 1;
            }
        }
    }
    __syncthreads();                                   // M_r is done with: the tile's normalised rows go over it
    stage_rows<DP>(ent, ld, dim, l2n, pos, neg, items, count, tile, Xs);
    __syncthreads();
    // dM = dY^T X over the tile's rows: wave w owns the output row blocks w and w + 4
    const bool single = ws.rel_ntiles[r] == 1;
    float *mr = rel_matrix + r * dd, *ar = rel_matrix_acc ? rel_matrix_acc + r * dd : nullptr;
    float *slab = ws.slab + (int64_t)blockIdx.x * dd;
    const int kc = (count + 3) & ~3;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int jb = wave + 4 * h;
        if (jb >= NCB) continue;
        f32x4 acc[NCB];
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float *ap = Ds + (lane >> 4) * S + 16 * jb + (lane & 15);    // A[j][i] = dY[i][j]
        const float *bp = Xs + (lane >> 4) * S + (lane & 15);              // B[i][k] = X[i][k]
        for (int ii = 0; ii < kc; ii += 4) {
            const float a = ap[ii * S];
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bp[ii * S + 16 * cb], acc[cb], 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = 16 * jb + 4 * (lane >> 4) + q;
            if (j >= dim) continue;
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) {
                const int k = 16 * cb + (lane & 15);
                if (k >= dim) continue;
                const int64_t idx = (int64_t)j * dim + k;
                if (single) matrix_update(mr + idx, ar ? ar + idx : nullptr, acc[cb][q], lr, adagrad);
                else slab[idx] = acc[cb][q];
            }
        }
    }
}

// relations with more than one tile: slabs summed in tile order, then the optimiser; grid (ceil(d*d / 256), n_rel)
__global__ __launch_bounds__(256) void mapply_kernel(float *__restrict__ rel_matrix, float *__restrict__ rel_matrix_acc, int64_t dd,
                                                     TrWs ws, float lr, int adagrad) {
    const int64_t r = blockIdx.y, e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int nt = ws.rel_ntiles[r];
    if (nt <= 1 || e >= dd) return;
    const int t0 = ws.rel_tile0[r];
    float g = 0.f;
    for (int t = 0; t < nt; ++t) g += ws.slab[(int64_t)(t0 + t) * dd + e];
    const int64_t idx = r * dd + e;
    matrix_update(rel_matrix + idx, rel_matrix_acc ? rel_matrix_acc + idx : nullptr, g, lr, adagrad);
}

template <int DP>
int launch_tiles(const float *ent, int ld, int dim, const oea_step_cfg &cfg, float *rel_matrix, float *rel_matrix_acc,
                 const int32_t *pos, const int32_t *neg, const TrWs &ws, unsigned grid, oea::grad_t *ent_grad,
                 oea::flag_t *ent_touched, int which, hipStream_t st) {
    constexpr int S = DP + 4;
    const int tile = T;
    if (which == 0) {
        const size_t lds = sizeof(float) * (size_t)(DP + tile) * S;
        static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&fwd_kernel<DP>),
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        OEA_CHECK_HIP(attr);
        fwd_kernel<DP><<<grid, 256, lds, st>>>(ent, ld, dim, cfg.ent_l2_norm, rel_matrix, pos, neg, ws, tile);
    } else {
        const size_t lds = sizeof(float) * (size_t)((DP > tile ? DP : tile) + tile) * S;
        static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&bwd_kernel<DP>),
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        OEA_CHECK_HIP(attr);
        bwd_kernel<DP><<<grid, 256, lds, st>>>(ent, ld, dim, cfg.ent_l2_norm, rel_matrix, rel_matrix_acc, pos, neg, ws, ent_grad,
                                               ent_touched, cfg.lr, cfg.opt_kind == OEA_OPT_ADAGRAD, tile);
    }
    return OEA_OK;
}

}  // namespace

extern "C" {

size_t oea_transr_workspace_bytes(int64_t n_ent, int64_t n_rel, int32_t dim, int64_t max_pos) {
    (void)n_ent;
    if (n_rel < 0 || dim <= 0 || max_pos < 0) return 0;
    return tr_layout(n_rel, dim, max_pos, nullptr, nullptr);
}

int oea_transr_step(float *ent, float *ent_acc, int64_t n_ent, float *rel, float *rel_acc, int64_t n_rel, float *rel_matrix,
                    float *rel_matrix_acc, int32_t dim, int32_t ld, const int32_t *pos, int64_t n_pos, const int32_t *neg,
                    int64_t n_neg, const oea_step_cfg *cfg, void *step_workspace, void *transr_workspace, double *loss_accum,
                    void *stream) {
    OEA_REQUIRE(ent && rel && rel_matrix && cfg && step_workspace && transr_workspace && loss_accum, "null pointer");
    OEA_REQUIRE(n_pos >= 0 && (pos || n_pos == 0) && (neg || n_neg == 0), "pos / neg");
    OEA_REQUIRE(cfg->score_kind == OEA_SCORE_TRANSE, "TransR takes score_kind = OEA_SCORE_TRANSE (the projection is its own)");
    OEA_REQUIRE(cfg->loss_kind == OEA_LOSS_MARGIN && cfg->l1 == 0, "TransR: margin-based loss with loss_norm L2");
    OEA_REQUIRE(n_neg == n_pos, "the margin loss pairs pos i with neg i");
    OEA_REQUIRE(cfg->neg_group_k == 0 || cfg->neg_group_k == 1, "one negative per positive");
    OEA_REQUIRE(cfg->opt_kind == OEA_OPT_SGD || cfg->opt_kind == OEA_OPT_ADAGRAD, "TransR: SGD or Adagrad");
    OEA_REQUIRE(cfg->opt_kind == OEA_OPT_SGD || (ent_acc && rel_acc && rel_matrix_acc), "Adagrad needs its three accumulators");
    OEA_REQUIRE(dim > 0 && dim <= ld && ld % 4 == 0, "0 < dim <= ld, ld % 4 == 0");
    if (dim > kMaxDim) {
        oea::set_error("TransR: dim %d > %d (M_r is staged whole in LDS)", dim, kMaxDim);
        return OEA_EUNSUPPORTED;
    }
    OEA_REQUIRE(4 * n_pos < (int64_t)1 << 31, "4 n_pos < 2^31");
    hipStream_t st = oea::as_stream(stream);
    if (n_pos > 0 && n_rel > 0) {
        int rc = OEA_OK;
        grad_t *ent_grad, *rel_grad;
        flag_t *ent_touched, *rel_touched;
        oea::step_scratch_rows(step_workspace, n_ent, n_rel, ld, &ent_grad, &ent_touched, &rel_grad, &rel_touched);
        TrWs ws;
        tr_layout(n_rel, dim, n_pos, transr_workspace, &ws);
        const int64_t N = 4 * n_pos, nb = oea::ceil_div(N, SB), mt = max_tiles(N, n_rel);
        OEA_REQUIRE(mt < 65536 * 32, "tile count");
        OEA_CHECK_HIP(hipMemsetAsync(ws.hist, 0, sizeof(int32_t) * (size_t)(nb * n_rel), st));
        rank_kernel<<<(unsigned)nb, SB, 0, st>>>(pos, neg, N, n_rel, ws.hist, ws.rank);
        scan_kernel<<<1, 1024, 0, st>>>(ws.hist, nb, n_rel, ws.rel_tile0, ws.rel_ntiles, ws.n_tiles, ws.tiles, T);
        scatter_kernel<<<(unsigned)nb, SB, 0, st>>>(pos, neg, N, n_rel, ws.hist, ws.rank, ws.sorted);
#define OEA_TILES(DP, WHICH) rc = launch_tiles<DP>(ent, ld, dim, *cfg, rel_matrix, rel_matrix_acc, pos, neg, ws, (unsigned)mt, ent_grad, \
                                                   ent_touched, WHICH, st)
#define OEA_TR_DISPATCH(WHICH)                                                                 \
        switch (dpad(dim)) {                                                                   \
            case 16: OEA_TILES(16, WHICH); break;                                              \
            case 32: OEA_TILES(32, WHICH); break;                                              \
            case 48: OEA_TILES(48, WHICH); break;                                              \
            case 64: OEA_TILES(64, WHICH); break;                                              \
            case 80: OEA_TILES(80, WHICH); break;                                              \
            case 96: OEA_TILES(96, WHICH); break;                                              \
            case 112: OEA_TILES(112, WHICH); break;                                            \
            default: OEA_TILES(128, WHICH); break;                                             \
        }                                                                                      \
        if (rc != OEA_OK) return rc;
        OEA_TR_DISPATCH(0)
        const unsigned nl = (unsigned)oea::ceil_div(n_pos, 4);
        switch (dpad(dim)) {
            case 16: loss_kernel<16><<<nl, 256, 0, st>>>(rel, ld, dim, cfg->rel_l2_norm, pos, neg, n_pos, cfg->margin, ws, rel_grad, rel_touched, loss_accum); break;
            case 32: loss_kernel<32><<<nl, 256, 0, st>>>(rel, ld, dim, cfg->rel_l2_norm, pos, neg, n_pos, cfg->margin, ws, rel_grad, rel_touched, loss_accum); break;
            case 48: loss_kernel<48><<<nl, 256, 0, st>>>(rel, ld, dim, cfg->rel_l2_norm, pos, neg, n_pos, cfg->margin, ws, rel_grad, rel_touched, loss_accum); break;
            case 64: loss_kernel<64><<<nl, 256, 0, st>>>(rel, ld, dim, cfg->rel_l2_norm, pos, neg, n_pos, cfg->margin, ws, rel_grad, rel_touched, loss_accum); break;
            case 80: loss_kernel<80><<<nl, 256, 0, st>>>(rel, ld, dim, cfg->rel_l2_norm, pos, neg, n_pos, cfg->margin, ws, rel_grad, rel_touched, loss_accum); break;
            case 96: loss_kernel<96><<<nl, 256, 0, st>>>(rel, ld, dim, cfg->rel_l2_norm, pos, neg, n_pos, cfg->margin, ws, rel_grad, rel_touched, loss_accum); break;
            case 112: loss_kernel<112><<<nl, 256, 0, st>>>(rel, ld, dim, cfg->rel_l2_norm, pos, neg, n_pos, cfg->margin, ws, rel_grad, rel_touched, loss_accum); break;
            default: loss_kernel<128><<<nl, 256, 0, st>>>(rel, ld, dim, cfg->rel_l2_norm, pos, neg, n_pos, cfg->margin, ws, rel_grad, rel_touched, loss_accum); break;
        }
        OEA_TR_DISPATCH(1)
#undef OEA_TR_DISPATCH
#undef OEA_TILES
        const int64_t dd = (int64_t)dim * dim;
        mapply_kernel<<<dim3((unsigned)oea::ceil_div(dd, 256), (unsigned)n_rel), 256, 0, st>>>(
            rel_matrix, rel_matrix_acc, dd, ws, cfg->lr, cfg->opt_kind == OEA_OPT_ADAGRAD);
        OEA_CHECK_HIP(hipGetLastError());
    }
    // entity / relation rows: the step engine's optimiser on what the kernels above put into its scratch
    return oea_triple_step_phase(ent, ent_acc, n_ent, rel, rel_acc, n_rel, dim, ld, nullptr, 0, nullptr, 0, cfg, step_workspace,
                                 loss_accum, OEA_PHASE_APPLY, stream);
}

}  // extern "C"
