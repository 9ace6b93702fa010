// l1_grid.hip -- the manhattan metric through a 16-bit grid (RDGCN / GCN-Align: similarity.py:46-48, alignment.py:146-168).
//
// This file holds: the rows of a table on a common u16 grid (oea_quantize_rows_u16), strips of grid distances with v_sad_u16
// (oea_l1_u16_strip), the alignment ranks from such a strip with the undecided candidates settled by the exact fp64 chain
// (oea_rank_l1_grid_rows, _csls), and the exact distances of listed pairs (oea_pair_l1_sim, oea_pair_l1_f64).  The all-pairs fp64
// sweep these replace, and whose bits they reproduce, is rank_valu_kernel in sim_rank.hip.  No matrix cores here.
#include "sim_tiles.h"

using oea::f2ord;              // order-preserving float -> uint (sim_tiles.h: the one thing this file takes from it)

namespace {

constexpr int LT = 128;        // strip tile edge: 128 x 128 per workgroup, 8 x 8 per thread (as sim_l1_f32_store_kernel, sim_rank.hip)

// ---- fixed-point L1 pre-filter: rows on a common u16 grid, v_sad_u16 (two columns per instruction) -----------------------
// q = round((x - lo) * inv_step) in 0..65535 with lo / step from the table's own range: |x - (lo + q step)| <= step / 2, so
// the grid distance  step * sum_k |qa_k - qb_k|  is within dim * step of the true L1 distance -- a bound the caller turns
// into a certificate (approaches/rdgcn.py:get_neg): a candidate list is accepted only if no row outside it can beat its
// k-th exact distance.  The fp32 kernel (sim_l1_f32_store_kernel, sim_rank.hip) issues 2 vector instructions per (pair, column) and runs at the full
// unpacked issue rate (61 ms for 20,000 x 200,000 x 300); this one issues 1/2.
__global__ __launch_bounds__(256) void quantize_rows_u16_kernel(const float *__restrict__ src, int64_t n, int ld, int dim, float lo,
                                                                float inv_step, uint16_t *__restrict__ dst, int ldq) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;       // one thread per 8 columns (one 16-byte store)
    const int per_row = ldq >> 3;
    if (idx >= n * per_row) return;
    const int64_t row = idx / per_row;
    const int k0 = (int)(idx % per_row) * 8;
    uint32_t w[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        uint32_t h[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int k = k0 + 2 * e + u;
            float v = 0.f;                                                   // pad columns: the same grid point in every row
            if (k < dim) v = fminf(fmaxf(rintf((src[row * ld + k] - lo) * inv_step), 0.f), 65535.f);
            h[u] = (uint32_t)v;
        }
        w[e] = h[0] | (h[1] << 16);
    }
    *reinterpret_cast<uint4 *>(dst + row * ldq + k0) = make_uint4(w[0], w[1], w[2], w[3]);
}

// out[i, j] = -(float) sum_k |q[i, k] - c[j, k]|  (larger = nearer, what oea_topk_rows selects).  Same tiling as
// sim_l1_f32_store_kernel: 128 x 128 per workgroup, 8 x 8 per thread, operands k-major in LDS as dwords of two columns.
constexpr int UK = 32;                                                       // dwords (64 columns) per staged chunk
__global__ __launch_bounds__(256) void l1_u16_strip_kernel(const uint16_t *__restrict__ q, int64_t nq,
                                                           const uint16_t *__restrict__ c, int64_t nc, int ldq,
                                                           float *__restrict__ out, int64_t ld_out) {
    __shared__ __attribute__((aligned(16))) uint32_t Qs[UK * LT];
    __shared__ __attribute__((aligned(16))) uint32_t Cs[UK * LT];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t q0 = (int64_t)blockIdx.y * LT, c0 = (int64_t)blockIdx.x * LT;
    uint32_t acc[8][8];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) acc[a][b] = 0u;
    const int r = tid >> 1, wq = (tid & 1) * 16;                              // staging: thread -> (row, 16 dwords of the chunk)
    const int ldw = ldq >> 1;                                                // dwords per row, a multiple of 4
    const uint32_t *qrow = reinterpret_cast<const uint32_t *>(q) + (q0 + r) * ldw;
    const uint32_t *crow = reinterpret_cast<const uint32_t *>(c) + (c0 + r) * ldw;
    const bool q_in = q0 + r < nq, c_in = c0 + r < nc;
    for (int w0 = 0; w0 < ldw; w0 += UK) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 16; e += 4) {
            const int w = w0 + wq + e;
            uint4 qv = make_uint4(0u, 0u, 0u, 0u), cv = make_uint4(0u, 0u, 0u, 0u);
            if (q_in && w < ldw) qv = *reinterpret_cast<const uint4 *>(qrow + w);
            if (c_in && w < ldw) cv = *reinterpret_cast<const uint4 *>(crow + w);
            Qs[(wq + e + 0) * LT + r] = qv.x; Qs[(wq + e + 1) * LT + r] = qv.y; Qs[(wq + e + 2) * LT + r] = qv.z; Qs[(wq + e + 3) * LT + r] = qv.w;
            Cs[(wq + e + 0) * LT + r] = cv.x; Cs[(wq + e + 1) * LT + r] = cv.y; Cs[(wq + e + 2) * LT + r] = cv.z; Cs[(wq + e + 3) * LT + r] = cv.w;
        }
        __syncthreads();
        const int kk = min(UK, ldw - w0);
        for (int k = 0; k < kk; ++k) {
            const uint4 qa = *reinterpret_cast<const uint4 *>(Qs + k * LT + ty * 4);
            const uint4 qb = *reinterpret_cast<const uint4 *>(Qs + k * LT + 64 + ty * 4);
            const uint4 ca = *reinterpret_cast<const uint4 *>(Cs + k * LT + tx * 4);
            const uint4 cb = *reinterpret_cast<const uint4 *>(Cs + k * LT + 64 + tx * 4);
            const uint32_t qv[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
            const uint32_t cv[8] = {ca.x, ca.y, ca.z, ca.w, cb.x, cb.y, cb.z, cb.w};
#pragma unroll
            for (int a = 0; a < 8; ++a)
#pragma unroll
                for (int b = 0; b < 8; ++b) acc[a][b] = __builtin_amdgcn_sad_u16(qv[a], cv[b], acc[a][b]);
        }
    }
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        const int64_t i = q0 + (a < 4 ? ty * 4 + a : 64 + ty * 4 + (a - 4));
        if (i >= nq) continue;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int64_t j = c0 + h * 64 + tx * 4;
            float *o = out + i * ld_out + j;
            if (j + 3 < nc && (ld_out & 3) == 0) {
                oea::st4(o, make_float4(-(float)acc[a][h * 4 + 0], -(float)acc[a][h * 4 + 1], -(float)acc[a][h * 4 + 2], -(float)acc[a][h * 4 + 3]));
            } else {
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (j + b < nc) o[b] = -(float)acc[a][h * 4 + b];
            }
        }
    }
}

// ---- manhattan evaluation from the grid distances (RDGCN's metric, similarity.py:46-48 + alignment.py:146-168) -------------
// The reference ranks float32(1 - cdist(e1, e2, 'cityblock')): fp64 distances of EVERY pair (rank_valu_kernel: 125 ms at
// 70,000^2 x 300, the fp64 vector rate).  Here every pair only gets its 16-bit grid distance G (l1_u16_strip_kernel); the
// true distance lies within `err` of G step, so against the gold distance d_g a candidate is
//     certainly nearer   G step + err < d_g      -> counted,
//     certainly farther  G step - err > d_g      -> ignored,
//     in between                                  -> its EXACT similarity decides (sequential fp64 chain, the bits of
//                                                    rank_valu_kernel / scipy), tie rule included;
// the nearest candidate is the best exact similarity among the candidates within 2 err of the smallest grid distance.
// One workgroup per query row over its strip row [nc] of -G (two reads, the second out of L2); the few exact distances
// are one thread each.  A row whose candidate lists overflow (cannot happen unless thousands of candidates sit within
// `err` of the gold distance) evaluates every pair exactly.
constexpr int kGridAmb = 2048, kGridTop = 4096;

__device__ __forceinline__ float exact_l1_sim(const double *__restrict__ qs, const float *__restrict__ c, int dim) {
    double acc = 0.0;
#pragma unroll 4
    for (int k = 0; k < dim; ++k) acc += fabs(qs[k] - (double)c[k]);       // k ascending: valu_tile's order
    return (float)(1.0 - acc);
}

__global__ __launch_bounds__(256) void rank_l1_grid_rows_kernel(const float *__restrict__ strip, int64_t rows, int64_t row0, int64_t nc,
                                                                int64_t ld, const float *__restrict__ e1, int ld1,
                                                                const float *__restrict__ e2, int ld2, int dim, int64_t gold_off,
                                                                float step, float err, int32_t *__restrict__ rank,
                                                                int32_t *__restrict__ argmax, int32_t *__restrict__ n_exact_rows) {
    extern __shared__ double lds_d[];                              // qs [dim] (padded to even), then the lists
    double *qs = lds_d;
    int32_t *amb = reinterpret_cast<int32_t *>(qs + ((dim + 1) & ~1));
    int32_t *top = amb + kGridAmb;
    __shared__ int s_namb, s_ntop, s_cnt;
    __shared__ float s_gold, s_gmin;
    __shared__ unsigned long long s_best;
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    if (r >= rows) return;
    const int64_t i = row0 + r, g = i + gold_off;
    for (int k = tid; k < dim; k += 256) qs[k] = (double)e1[i * ld1 + k];
    if (tid == 0) { s_namb = 0; s_ntop = 0; s_cnt = 0; s_best = 0ull; s_gmin = INFINITY; }
    __syncthreads();
    if (tid == 0) s_gold = exact_l1_sim(qs, e2 + g * ld2, dim);
    __syncthreads();
    const float sg = s_gold;
    // slack: the float rounding of the similarities around the gold one and of grid sums >= 2^24
    const float tol = err + 4.0e-7f * fmaxf(fabsf(sg), 1.0f) + 4.0f * step;
    const float dg = (float)(1.0 - (double)sg);
    const float g_lo = (dg - tol) / step, g_hi = (dg + tol) / step;          // in grid units; strip holds -G
    const float *srow = strip + r * ld;
    const float band = 2.0f * tol / step;
    int cnt = 0;
    float gmin = INFINITY;
    // ONE read of the strip row: the candidates for the nearest are collected against the thread's RUNNING minimum (a
    // superset of those within `band` of the row's minimum: ~ln(n / 256) records per thread on unordered data) and filtered
    // once the row minimum is known; only if that list overflows (candidates ordered by falling distance) the row is read again
    for (int64_t j4 = (int64_t)tid * 4; j4 < nc; j4 += 1024) {       // ld % 4 == 0: 16-byte reads; columns >= nc are unwritten
        const float4 v4 = oea::ld4(srow + j4);
        const float Gs[4] = {-v4.x, -v4.y, -v4.z, -v4.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t j = j4 + u;
            const float G = Gs[u];
            if (j >= nc) continue;
            if (G <= gmin + band) {
                const int at = atomicAdd(&s_ntop, 1);
                if (at < kGridTop) top[at] = (int32_t)j;
            }
            gmin = fminf(gmin, G);
            if (j == g) continue;
            if (G < g_lo) ++cnt;
            else if (G <= g_hi) {
                const int at = atomicAdd(&s_namb, 1);
                if (at < kGridAmb) amb[at] = (int32_t)j;
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        cnt += __shfl_xor(cnt, off, 64);
        gmin = fminf(gmin, __shfl_xor(gmin, off, 64));
    }
    if ((tid & 63) == 0) {
        atomicAdd(&s_cnt, cnt);
        atomicMin(reinterpret_cast<int *>(&s_gmin), __float_as_int(gmin));     // G >= 0: the int order is the float order
    }
    __syncthreads();
    const float top_hi = s_gmin + band;
    if (s_ntop > kGridTop) {                                        // workgroup-uniform
        __syncthreads();
        if (tid == 0) s_ntop = 0;
        __syncthreads();
        for (int64_t j = tid; j < nc; j += 256) {
            if (-srow[j] <= top_hi) {
                const int at = atomicAdd(&s_ntop, 1);
                if (at < kGridTop) top[at] = (int32_t)j;
            }
        }
        __syncthreads();
    }
    const int namb = s_namb, ntop = s_ntop;
    int extra = 0;
    unsigned long long best = 0ull;
    if (namb > kGridAmb || ntop > kGridTop) {
        // every pair exactly (the lists overflowed); counted, so that the caller can leave the grid path when a table's
        // range makes its error bound useless (a few outliers stretch the grid: most candidates become doubtful)
        if (tid == 0 && n_exact_rows) atomicAdd(n_exact_rows, 1);
        for (int64_t j = tid; j < nc; j += 256) {
            const float v = exact_l1_sim(qs, e2 + j * ld2, dim);
            extra += (j != g) && (v > sg || (v == sg && j < g));
            const unsigned long long key = ((unsigned long long)f2ord(v) << 32) | (0xFFFFFFFFu - (uint32_t)j);
            best = key > best ? key : best;
        }
        __syncthreads();
        if (tid == 0) s_cnt = 0;                                    // the grid count is replaced, not extended
        __syncthreads();
    } else {
        for (int a = tid; a < namb; a += 256) {
            const int64_t j = amb[a];
            const float v = exact_l1_sim(qs, e2 + j * ld2, dim);
            extra += v > sg || (v == sg && j < g);
        }
        for (int a = tid; a < ntop; a += 256) {
            const int64_t j = top[a];
            if (-srow[j] > top_hi) continue;                        // a record of the running minimum only
            const float v = exact_l1_sim(qs, e2 + j * ld2, dim);
            const unsigned long long key = ((unsigned long long)f2ord(v) << 32) | (0xFFFFFFFFu - (uint32_t)j);
            best = key > best ? key : best;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        extra += __shfl_xor(extra, off, 64);
        const unsigned long long o = __shfl_xor(best, off, 64);
        best = o > best ? o : best;
    }
    if ((tid & 63) == 0) {
        if (extra) atomicAdd(&s_cnt, extra);
        atomicMax(&s_best, best);
    }
    __syncthreads();
    if (tid == 0) {
        rank[i] = s_cnt;
        argmax[i] = (int32_t)(0xFFFFFFFFu - (uint32_t)(s_best & 0xFFFFFFFFull));
    }
}

// ---- the same with CSLS (basic_model.py:132-135: test() runs greedy_alignment a second time with csls = args.csls; for
// GCN-Align / RDGCN that is the manhattan metric) ------------------------------------------------------------------------------
// v_ij = (2 s_ij - r_i) - c_j in fp32 (rank_valu_kernel's expression; s_ij = float(1 - d_ij)).  From the grid distance G the
// similarity is known to +-err, so v~_ij = (2 (1 - G step) - r_i) - c_j is within tol_j = 2 err + rounding slack of v_ij:
// candidates whose interval [v~ - tol, v~ + tol] does not contain the gold value are decided by the strip, the others -- and
// the candidates whose upper bound reaches the row's best lower bound, for the nearest -- by their exact value.
__device__ __forceinline__ float csls_tol(float s_approx, float r, float c, float err, float step) {
    return 2.0f * err + 8.0f * step + 6.0e-7f * (2.0f * fabsf(s_approx) + fabsf(r) + fabsf(c) + 1.0f);
}

__global__ __launch_bounds__(256) void rank_l1_grid_rows_csls_kernel(const float *__restrict__ strip, int64_t rows, int64_t row0,
                                                                     int64_t nc, int64_t ld, const float *__restrict__ e1, int ld1,
                                                                     const float *__restrict__ e2, int ld2, int dim, int64_t gold_off,
                                                                     float step, float err, const float *__restrict__ csls_r,
                                                                     const float *__restrict__ csls_c, int32_t *__restrict__ rank,
                                                                     int32_t *__restrict__ argmax, int32_t *__restrict__ n_exact_rows) {
    extern __shared__ double lds_d[];
    double *qs = lds_d;
    int32_t *amb = reinterpret_cast<int32_t *>(qs + ((dim + 1) & ~1));
    int32_t *top = amb + kGridAmb;
    __shared__ int s_namb, s_ntop, s_cnt;
    __shared__ float s_gold;
    __shared__ unsigned s_lmax_ord;                                  // f2ord bits of the row's best lower bound
    __shared__ unsigned long long s_best;
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    if (r >= rows) return;
    const int64_t i = row0 + r, g = i + gold_off;
    const float ri = csls_r[i];
    for (int k = tid; k < dim; k += 256) qs[k] = (double)e1[i * ld1 + k];
    if (tid == 0) { s_namb = 0; s_ntop = 0; s_cnt = 0; s_best = 0ull; s_lmax_ord = 0u; }
    __syncthreads();
    if (tid == 0) s_gold = (2.0f * exact_l1_sim(qs, e2 + g * ld2, dim) - ri) - csls_c[g];
    __syncthreads();
    const float vg = s_gold;
    const float *srow = strip + r * ld;
    int cnt = 0;
    float lmax = -INFINITY;                                          // running maximum of the lower bounds v~ - tol
    for (int64_t j4 = (int64_t)tid * 4; j4 < nc; j4 += 1024) {       // ld % 4 == 0: 16-byte reads; columns >= nc are unwritten
        const float4 v4 = oea::ld4(srow + j4);
        const float Gs[4] = {-v4.x, -v4.y, -v4.z, -v4.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t j = j4 + u;
            if (j >= nc) continue;
            const float cj = csls_c[j];
            const float sa = fmaf(-Gs[u], step, 1.0f);
            const float va = (2.0f * sa - ri) - cj;
            const float tol = csls_tol(sa, ri, cj, err, step);
            if (va + tol >= lmax) {
                const int at = atomicAdd(&s_ntop, 1);
                if (at < kGridTop) top[at] = (int32_t)j;
            }
            lmax = fmaxf(lmax, va - tol);
            if (j == g) continue;
            if (va - tol > vg) ++cnt;
            else if (va + tol >= vg) {
                const int at = atomicAdd(&s_namb, 1);
                if (at < kGridAmb) amb[at] = (int32_t)j;
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        cnt += __shfl_xor(cnt, off, 64);
        lmax = fmaxf(lmax, __shfl_xor(lmax, off, 64));
    }
    if ((tid & 63) == 0) {
        atomicAdd(&s_cnt, cnt);
        atomicMax(&s_lmax_ord, f2ord(lmax));                         // order-preserving bits: the bound may be negative
    }
    __syncthreads();
    float row_lmax;
    {
        const unsigned o = s_lmax_ord;
        row_lmax = __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
    }
    auto upper = [&](int64_t j) {
        const float cj = csls_c[j];
        const float sa = fmaf(srow[j], step, 1.0f);                   // srow holds -G
        return ((2.0f * sa - ri) - cj) + csls_tol(sa, ri, cj, err, step);
    };
    if (s_ntop > kGridTop) {                                        // workgroup-uniform
        __syncthreads();
        if (tid == 0) s_ntop = 0;
        __syncthreads();
        for (int64_t j = tid; j < nc; j += 256) {
            if (upper(j) >= row_lmax) {
                const int at = atomicAdd(&s_ntop, 1);
                if (at < kGridTop) top[at] = (int32_t)j;
            }
        }
        __syncthreads();
    }
    const int namb = s_namb, ntop = s_ntop;
    int extra = 0;
    unsigned long long best = 0ull;
    if (namb > kGridAmb || ntop > kGridTop) {                        // the lists overflowed: every pair exactly
        if (tid == 0 && n_exact_rows) atomicAdd(n_exact_rows, 1);
        for (int64_t j = tid; j < nc; j += 256) {
            const float v = (2.0f * exact_l1_sim(qs, e2 + j * ld2, dim) - ri) - csls_c[j];
            extra += (j != g) && (v > vg || (v == vg && j < g));
            const unsigned long long key = ((unsigned long long)f2ord(v) << 32) | (0xFFFFFFFFu - (uint32_t)j);
            best = key > best ? key : best;
        }
        __syncthreads();
        if (tid == 0) s_cnt = 0;
        __syncthreads();
    } else {
        for (int a = tid; a < namb; a += 256) {
            const int64_t j = amb[a];
            const float v = (2.0f * exact_l1_sim(qs, e2 + j * ld2, dim) - ri) - csls_c[j];
            extra += v > vg || (v == vg && j < g);
        }
        for (int a = tid; a < ntop; a += 256) {
            const int64_t j = top[a];
            if (upper(j) < row_lmax) continue;                       // a record of the running bound only
            const float v = (2.0f * exact_l1_sim(qs, e2 + j * ld2, dim) - ri) - csls_c[j];
            const unsigned long long key = ((unsigned long long)f2ord(v) << 32) | (0xFFFFFFFFu - (uint32_t)j);
            best = key > best ? key : best;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        extra += __shfl_xor(extra, off, 64);
        const unsigned long long o = __shfl_xor(best, off, 64);
        best = o > best ? o : best;
    }
    if ((tid & 63) == 0) {
        if (extra) atomicAdd(&s_cnt, extra);
        atomicMax(&s_best, best);
    }
    __syncthreads();
    if (tid == 0) {
        rank[i] = s_cnt;
        argmax[i] = (int32_t)(0xFFFFFFFFu - (uint32_t)(s_best & 0xFFFFFFFFull));
    }
}

// exact similarity float(1 - d) of every (query row, candidate) pair of a candidate list with the SEQUENTIAL fp64 chain
// (k ascending: the bits of valu_tile / scipy's cdist): one thread per pair.  The CSLS means of the manhattan metric are
// sums of these values, so the chain's order matters (pair_l1_f64_kernel below adds in a butterfly order).
__global__ __launch_bounds__(256) void pair_l1_sim_seq_kernel(const float *__restrict__ q, int64_t nq, int ldq,
                                                              const float *__restrict__ table, int ldt, int dim,
                                                              const int32_t *__restrict__ cand, int c, float *__restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nq * c) return;
    const float *a = q + (p / c) * ldq, *b = table + (int64_t)cand[p] * ldt;
    double acc = 0.0;
#pragma unroll 4
    for (int k = 0; k < dim; ++k) acc += fabs((double)a[k] - (double)b[k]);
    out[p] = (float)(1.0 - acc);
}

// exact fp64 L1 distance of every (query row, candidate) pair of a candidate list: one 16-lane group per pair, lane-strided
// columns, butterfly sum (a fixed order: equal rows give equal sums)
__global__ __launch_bounds__(256) void pair_l1_f64_kernel(const float *__restrict__ q, int64_t nq, int ldq,
                                                          const float *__restrict__ table, int ldt, int dim,
                                                          const int32_t *__restrict__ cand, int c, double *__restrict__ out) {
    const int lane = threadIdx.x & 15;
    const int64_t p = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    if (p >= nq * c) return;
    const int64_t i = p / c;
    const float *a = q + i * ldq, *b = table + (int64_t)cand[p] * ldt;
    double s = 0.0;
    for (int k = lane; k < dim; k += 16) s += fabs((double)a[k] - (double)b[k]);
    s = oea::group_sum_d<16>(s);
    if (lane == 0) out[p] = s;
}

}  // namespace

extern "C" {

int oea_quantize_rows_u16(const float *src, int64_t n, int32_t ld, int32_t dim, float lo, float inv_step, uint16_t *dst,
                          int32_t ldq, void *stream) {
    OEA_REQUIRE(src && dst && dim > 0 && dim <= ld && ldq % 8 == 0 && dim <= ldq && n >= 0, "ldq: a multiple of 8 >= dim");
    if (n == 0) return OEA_OK;
    const int64_t items = n * (ldq / 8);
    quantize_rows_u16_kernel<<<(unsigned)oea::ceil_div(items, 256), 256, 0, oea::as_stream(stream)>>>(src, n, ld, dim, lo, inv_step,
                                                                                                 dst, ldq);
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

int oea_l1_u16_strip(const uint16_t *q, int64_t nq, const uint16_t *c, int64_t nc, int32_t ldq, float *out, int64_t ld_out,
                     void *stream) {
    OEA_REQUIRE(q && c && out && ldq > 0 && ldq % 8 == 0 && ld_out >= nc, "ldq: a multiple of 8; ld_out >= nc");
    OEA_REQUIRE(ldq <= 32768, "at most 32768 columns (u32 sums)");   // sums >= 2^24 round to float: <= 2^-24 relative
    if (nq == 0 || nc == 0) return OEA_OK;
    l1_u16_strip_kernel<<<dim3((unsigned)oea::ceil_div(nc, LT), (unsigned)oea::ceil_div(nq, LT)), 256, 0, oea::as_stream(stream)>>>(
        q, nq, c, nc, ldq, out, ld_out);
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

int oea_rank_l1_grid_rows(const float *strip, int64_t rows, int64_t row0, int64_t nc, int64_t ld, const float *e1, int32_t ld1,
                          const float *e2, int32_t ld2, int32_t dim, int64_t gold_offset, float step, float err, int32_t *rank,
                          int32_t *argmax, int32_t *n_exact_rows, void *stream) {
    OEA_REQUIRE(strip && e1 && e2 && rank && argmax && rows >= 0 && row0 >= 0 && nc > 0 && ld >= nc, "arguments");
    OEA_REQUIRE(ld % 4 == 0 && ((uintptr_t)strip & 15) == 0, "strip rows: 16-byte aligned (ld % 4 == 0)");
    OEA_REQUIRE(dim > 0 && dim <= ld1 && dim <= ld2 && dim <= 4096 && step > 0.f && err >= 0.f, "dim <= 4096, step > 0");
    OEA_REQUIRE(row0 + rows + gold_offset <= nc && gold_offset >= 0, "gold of row i is column gold_offset + i < nc");
    if (rows == 0) return OEA_OK;
    const size_t lds = sizeof(double) * (size_t)((dim + 1) & ~1) + sizeof(int32_t) * (kGridAmb + kGridTop);
    rank_l1_grid_rows_kernel<<<(unsigned)rows, 256, lds, oea::as_stream(stream)>>>(strip, rows, row0, nc, ld, e1, ld1, e2, ld2, dim,
                                                                                   gold_offset, step, err, rank, argmax, n_exact_rows);
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

int oea_rank_l1_grid_rows_csls(const float *strip, int64_t rows, int64_t row0, int64_t nc, int64_t ld, const float *e1, int32_t ld1,
                               const float *e2, int32_t ld2, int32_t dim, int64_t gold_offset, float step, float err,
                               const float *csls_r, const float *csls_c, int32_t *rank, int32_t *argmax, int32_t *n_exact_rows,
                               void *stream) {
    OEA_REQUIRE(strip && e1 && e2 && rank && argmax && csls_r && csls_c && rows >= 0 && row0 >= 0 && nc > 0 && ld >= nc, "arguments");
    OEA_REQUIRE(ld % 4 == 0 && ((uintptr_t)strip & 15) == 0, "strip rows: 16-byte aligned (ld % 4 == 0)");
    OEA_REQUIRE(dim > 0 && dim <= ld1 && dim <= ld2 && dim <= 4096 && step > 0.f && err >= 0.f, "dim <= 4096, step > 0");
    OEA_REQUIRE(row0 + rows + gold_offset <= nc && gold_offset >= 0, "gold of row i is column gold_offset + i < nc");
    if (rows == 0) return OEA_OK;
    const size_t lds = sizeof(double) * (size_t)((dim + 1) & ~1) + sizeof(int32_t) * (kGridAmb + kGridTop);
    rank_l1_grid_rows_csls_kernel<<<(unsigned)rows, 256, lds, oea::as_stream(stream)>>>(strip, rows, row0, nc, ld, e1, ld1, e2, ld2, dim,
                                                                                        gold_offset, step, err, csls_r, csls_c, rank,
                                                                                        argmax, n_exact_rows);
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

int oea_pair_l1_sim(const float *q, int64_t nq, int32_t ldq, const float *table, int64_t n, int32_t ldt, int32_t dim,
                    const int32_t *cand, int32_t c, float *out, void *stream) {
    OEA_REQUIRE(q && table && cand && out && dim > 0 && dim <= ldq && dim <= ldt && c > 0 && n > 0, "arguments");
    if (nq == 0) return OEA_OK;
    pair_l1_sim_seq_kernel<<<(unsigned)oea::ceil_div(nq * c, 256), 256, 0, oea::as_stream(stream)>>>(q, nq, ldq, table, ldt, dim, cand, c, out);
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

int oea_pair_l1_f64(const float *q, int64_t nq, int32_t ldq, const float *table, int64_t n, int32_t ldt, int32_t dim,
                    const int32_t *cand, int32_t c, double *out, void *stream) {
    OEA_REQUIRE(q && table && cand && out && dim > 0 && dim <= ldq && dim <= ldt && c > 0 && n > 0, "arguments");
    if (nq == 0) return OEA_OK;
    const int64_t groups = nq * c;
    pair_l1_f64_kernel<<<(unsigned)oea::ceil_div(groups, 16), 256, 0, oea::as_stream(stream)>>>(q, nq, ldq, table, ldt, dim, cand, c, out);
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

}  // extern "C"
