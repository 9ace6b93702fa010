// nce_half.h -- the sampled-softmax (NCE) half that the ProjE and the ConvE steps share: the two MFMA sweeps, the label rows,
// the candidate constants and reductions, the step scratch bookkeeping and the fp64 block-partial reduction.  Included by
// proje_step.hip and conve_step.hip ONLY (its kernels are compiled into whoever includes it); everything lives in an anonymous
// namespace (one copy per translation unit).  The row helpers and log Q come from row_ops.h.
#pragma once
#include "row_ops.h"

#include <algorithm>

namespace {

using oea::grad_t;
using namespace oea::row;

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kMaxDim = 128;
constexpr int LP = 128;            // row stride of the batch buffers (zero padded)
constexpr int LDT = 132;           // LDS row stride of an operand tile: float4 reads of 16 consecutive rows hit distinct banks
constexpr int PLD = 36;            // LDS row stride of the sigma tile
constexpr int kRows = 32;          // batch rows per block of the column reductions
constexpr int kTargetWgs = 1024;   // sweep workgroups aimed at (4 per CU)
constexpr int kMaxSplit = 16;
constexpr float kBnEps = 1e-3f;

static int split_of(int fixed_tiles, int streamed_tiles) {
    int s = (kTargetWgs + fixed_tiles - 1) / fixed_tiles;
    s = std::min(s, std::min(streamed_tiles, kMaxSplit));
    return std::max(s, 1);
}

struct Bufs {
    float *g_ent, *g_rel, *g_w, *g_b, *g_vec;
    grad_t *s_ent, *s_rel, *s_w, *s_b;
    int32_t *last_h, *last_r, *last_t, *last_s, *last_n;
    float *hn, *rn, *out, *x, *dxlab, *dx, *invh, *invr, *dtrue;
    double *p, *pc, *sums;
    float *pa, *pb, *rowsum;
    double *loss_a, *loss_l;
};

__device__ __forceinline__ void zero_row(float *g, grad_t *s, int64_t row, int ld, int lane) {
    for (int c = lane; c < ld; c += 64) { g[row * ld + c] = 0.f; s[row * ld + c] = 0; }
}

// wave i clears the rows of item i of the saved lists (the counts are read on the device: no host copy of the last call is kept)
__global__ __launch_bounds__(256) void clear_prev_kernel(Bufs W, int ld, int64_t cap) {
    const int lane = threadIdx.x & 63;
    const int nb = W.last_n[0], ns = W.last_n[1];
    for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < cap; i += (int64_t)gridDim.x * 4) {
        if (i < nb) {
            zero_row(W.g_ent, W.s_ent, W.last_h[i], ld, lane);
            zero_row(W.g_rel, W.s_rel, W.last_r[i], ld, lane);
            const int64_t t = W.last_t[i];
            zero_row(W.g_w, W.s_w, t, ld, lane);
            if (lane == 0) { W.g_b[t] = 0.f; W.s_b[t] = 0; }
        }
        if (i < ns) {
            const int64_t s = W.last_s[i];
            zero_row(W.g_w, W.s_w, s, ld, lane);
            if (lane == 0) { W.g_b[s] = 0.f; W.s_b[s] = 0; }
        }
    }
}

// sums[k][c] = sum over the blocks of p[blk][k][c]: eight interleaved chains per column (block b in chain b % 8, each in block
// order), then the chains in chain order -- a fixed order that does not leave one thread walking every block
constexpr int kChains = 8;
__global__ __launch_bounds__(LP * kChains) void finalize_kernel(const double *__restrict__ p, int nblk, int nk, double *__restrict__ sums) {
    __shared__ double part[kChains][LP];
    const int c = threadIdx.x & (LP - 1), g = threadIdx.x / LP;
    for (int k = 0; k < nk; ++k) {
        double s = 0.0;
        for (int b = g; b < nblk; b += kChains) s += p[((size_t)b * 4 + k) * LP + c];
        part[g][c] = s;
        __syncthreads();
        if (g == 0) {
            double t = 0.0;
            for (int j = 0; j < kChains; ++j) t += part[j][c];
            sums[k * LP + c] = t;
        }
        __syncthreads();
    }
}

struct Stat { float mean, istd; };
__device__ __forceinline__ Stat stat_of(double s, double ss, double inv_n) {
    const double m = s * inv_n, v = fmax(ss * inv_n - m * m, 0.0);
    Stat r;
    r.mean = (float)m;
    r.istd = (float)(1.0 / sqrt(v + (double)kBnEps));
    return r;
}

// stage 3, one wave per batch row: X = BN_out(out) (BN_OUT; otherwise X is read as the caller left it in W.x, zero from dim on),
// the label's logit, its loss and its share of every gradient
template <bool BN_OUT>
__global__ __launch_bounds__(256) void label_kernel(Bufs W, int n_pos, int dim, int ld, const float *__restrict__ beta_out,
                                                    const float *__restrict__ ent_w, const float *__restrict__ ent_b,
                                                    const int32_t *__restrict__ pos, const int64_t *__restrict__ num_tries, double inv_log_e1) {
    __shared__ double wl[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x * 4 + wave;
    double loss = 0.0;
    if (b < n_pos) {
        const int c = 2 * lane;
        float2 x = make_float2(0.f, 0.f);
        if (BN_OUT) {
            const double inv_n = 1.0 / (double)n_pos;
            const double *S = W.sums + 4 * LP;
            const Stat s0 = stat_of(S[c], S[LP + c], inv_n), s1 = stat_of(S[c + 1], S[LP + c + 1], inv_n);
            const float2 o = *reinterpret_cast<const float2 *>(W.out + (size_t)b * LP + c);
            if (c < dim) x.x = (o.x - s0.mean) * s0.istd + beta_out[c];
            if (c + 1 < dim) x.y = (o.y - s1.mean) * s1.istd + beta_out[c + 1];
            *reinterpret_cast<float2 *>(W.x + (size_t)b * LP + c) = x;
        } else {
            x = *reinterpret_cast<const float2 *>(W.x + (size_t)b * LP + c);
        }
        const int64_t t = pos[3 * b + 2];
        const float2 w = load2(ent_w + t * ld, dim, lane);
        const float lq = (float)log_q(t, (double)*num_tries, inv_log_e1);
        const float logit = dot2(x, w) + ent_b[t] - lq;
        loss = (double)softplus_f(-logit);                       // xent(x, 1) = softplus(-x)
        const float dt = sigmoid_f(logit) - 1.f;
        *reinterpret_cast<float2 *>(W.dxlab + (size_t)b * LP + c) = make_float2(dt * w.x, dt * w.y);
        if (c < dim) oea::grad_add(W.s_w + t * ld + c, dt * x.x);
        if (c + 1 < dim) oea::grad_add(W.s_w + t * ld + c + 1, dt * x.y);
        if (lane == 0) { oea::grad_add(W.s_b + t, dt); W.dtrue[b] = dt; }
    }
    if (lane == 0) wl[wave] = loss;
    __syncthreads();
    if (threadIdx.x == 0) W.loss_l[blockIdx.x] = (wl[0] + wl[1]) + (wl[2] + wl[3]);
}

// ---- the NCE sweeps --------------------------------------------------------------------------------------------------------------
struct SweepArgs {
    const float *f_src; const int32_t *f_ids; int f_ld; int n_f;     // fixed rows (ids: gather)
    const float *g_src; const int32_t *g_ids; int g_ld; int n_g;     // streamed rows
    const float *bias; const float *logq; const int32_t *cand_ids;   // logit offset of candidate j: bias[cand_ids[j]] - logq[j]
    int dim, n_split;
    float *partial;          // [split][fixed rows padded to 32][LP]
    float *rowsum;           // CAND_FIXED: [split][fixed rows padded]
    double *loss;            // !CAND_FIXED: [split][fixed tiles]
};

// 32 rows x LP columns into an operand tile, zero outside (rows >= n, columns >= dim): the zero padding IS the K tail
__device__ __forceinline__ void stage_tile(float *dst, const float *src, const int32_t *ids, int ld, int row0, int n, int dim, int lane) {
    const int c4 = (lane & 31) * 4;
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
        const int r = 2 * i + (lane >> 5), row = row0 + r;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < n && c4 < dim) {
            const int64_t gr = ids ? (int64_t)ids[row] : (int64_t)row;
            v = oea::ld4(src + gr * ld + c4);          // ld % 4 == 0 and c4 < dim <= ld: the float4 lies inside the row
            if (c4 + 1 >= dim) v.y = 0.f;
            if (c4 + 2 >= dim) v.z = 0.f;
            if (c4 + 3 >= dim) v.w = 0.f;
        }
        oea::st4(dst + r * LDT + c4, v);
    }
}

template <bool CAND_FIXED, int NT>
__global__ __launch_bounds__(64) void nce_sweep_kernel(SweepArgs A) {
    __shared__ __attribute__((aligned(16))) float Fs[32 * LDT];
    __shared__ __attribute__((aligned(16))) float Gs[32 * LDT];
    __shared__ __attribute__((aligned(16))) float Ps[32 * PLD];
    __shared__ float off_f[32], off_g[32], omb_f[32], omb_g[32];
    const int lane = threadIdx.x, half = lane >> 5, l32 = lane & 31;
    const int f0 = blockIdx.x * 32, split = blockIdx.y;
    const int n_gt = (A.n_g + 31) / 32;
    const int gt0 = (int)((int64_t)split * n_gt / A.n_split), gt1 = (int)((int64_t)(split + 1) * n_gt / A.n_split);
    const int k8 = (A.dim + 7) & ~7;
    stage_tile(Fs, A.f_src, A.f_ids, A.f_ld, f0, A.n_f, A.dim, lane);
    if (lane < 32) {
        const float a = (CAND_FIXED && f0 + lane < A.n_f) ? A.bias[A.cand_ids[f0 + lane]] - A.logq[f0 + lane] : 0.f;
        off_f[lane] = a;
        omb_f[lane] = 1.f / (1.f + expf(a));
    }
    f32x16 acc[NT];
#pragma unroll
    for (int y = 0; y < NT; ++y)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[y][r] = 0.f;
    float rowsum = 0.f;
    double loss = 0.0;
    for (int gt = gt0; gt < gt1; ++gt) {
        const int g0 = gt * 32;
        __syncthreads();                                   // the previous tile's reads of Gs / Ps are done
        stage_tile(Gs, A.g_src, A.g_ids, A.g_ld, g0, A.n_g, A.dim, lane);
        if (lane < 32) {
            const float a = (!CAND_FIXED && g0 + lane < A.n_g) ? A.bias[A.cand_ids[g0 + lane]] - A.logq[g0 + lane] : 0.f;
            off_g[lane] = a;
            omb_g[lane] = 1.f / (1.f + expf(a));           // 1 - sigma(a)
        }
        __syncthreads();
        // logits[f][g] = F_f . G_g: lane (row l32, half) takes columns 8 q + 4 half .. + 3 of both operands, MFMA i pairs column
        // 8 q + i (half 0) with 8 q + 4 + i (half 1): the same k permutation on both sides
        f32x16 lg;
#pragma unroll
        for (int r = 0; r < 16; ++r) lg[r] = 0.f;
        for (int q = 0; q < k8; q += 8) {
            const float4 a = oea::ld4(Fs + l32 * LDT + q + 4 * half), b = oea::ld4(Gs + l32 * LDT + q + 4 * half);
            lg = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, lg, 0, 0, 0);
            lg = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, lg, 0, 0, 0);
            lg = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, lg, 0, 0, 0);
            lg = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, lg, 0, 0, 0);
        }
        // lg[r]: row f = (r & 3) + 8 (r >> 2) + 4 half, column g = l32
        const bool g_on = g0 + l32 < A.n_g;
        const float og = off_g[l32], ob = omb_g[l32];
        float lsum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int f = (r & 3) + 8 * (r >> 2) + 4 * half;
            const bool on = g_on && f0 + f < A.n_f;
            const float xv = lg[r] + off_f[f] + og;
            // sigma(d + a) - sigma(a) = -(1 - sigma(a)) sigma(d + a) expm1(-d), a = the candidate's offset: every factor exact to
            // fp32 rounding
            const float sg = sigmoid_f(xv);
            Ps[f * PLD + l32] = on ? -((CAND_FIXED ? omb_f[f] : ob) * sg * expm1f(-lg[r])) : 0.f;
            if (!CAND_FIXED && on) lsum += softplus_f(xv);
        }
        loss += (double)lsum;
        __syncthreads();
        // acc[f][c] += sum_g sigma[f][g] G[g][c]: the tile's 32 terms are summed on their own and added to the running sum once,
        // so that a sum over thousands of candidates rounds at the running sum's magnitude once per tile, not once per term
        f32x16 tacc[NT];
#pragma unroll
        for (int y = 0; y < NT; ++y)
#pragma unroll
            for (int r = 0; r < 16; ++r) tacc[y][r] = 0.f;
#pragma unroll
        for (int q = 0; q < 32; q += 8) {
            const float4 pa = oea::ld4(Ps + l32 * PLD + q + 4 * half);
            const float pv[4] = {pa.x, pa.y, pa.z, pa.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float *gp = Gs + (q + 4 * half + i) * LDT + l32;
#pragma unroll
                for (int y = 0; y < NT; ++y) tacc[y] = __builtin_amdgcn_mfma_f32_32x32x2f32(pv[i], gp[32 * y], tacc[y], 0, 0, 0);
            }
        }
#pragma unroll
        for (int y = 0; y < NT; ++y) acc[y] += tacc[y];
        if (CAND_FIXED && lane < 32) {
            float s = 0.f;
#pragma unroll
            for (int g = 0; g < 32; g += 4) {
                const float4 v = oea::ld4(Ps + lane * PLD + g);
                s += (v.x + v.y) + (v.z + v.w);
            }
            rowsum += s;
        }
    }
    const size_t rows_p = (size_t)gridDim.x * 32;
    float *out = A.partial + ((size_t)split * rows_p + f0) * LP;
#pragma unroll
    for (int y = 0; y < NT; ++y)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int f = (r & 3) + 8 * (r >> 2) + 4 * half;
            out[(size_t)f * LP + 32 * y + l32] = acc[y][r];
        }
    if (CAND_FIXED) {
        if (lane < 32) A.rowsum[(size_t)split * rows_p + f0 + lane] = rowsum;
    } else {
        const double tot = oea::wave_sum_d(loss);
        if (lane == 0) A.loss[(size_t)split * gridDim.x + blockIdx.x] = tot;
    }
}

// the row-independent part of dX, c = sum_j sigma(b[s_j] - log Q(s_j)) W[s_j], as fp64 partials per tile of 32 candidates
__global__ __launch_bounds__(LP) void cand_const_kernel(Bufs W, const float *__restrict__ ent_w, const float *__restrict__ ent_b,
                                                        const int32_t *__restrict__ sampled, const float *__restrict__ logq, int n_s,
                                                        int dim, int ld) {
    const int c = threadIdx.x;
    const int j0 = blockIdx.x * 32, j1 = min(j0 + 32, n_s);
    double s = 0.0;
    if (c < dim)
        for (int j = j0; j < j1; ++j) {
            const int64_t e = sampled[j];
            const double a = (double)(ent_b[e] - logq[j]);          // the fp32 offset the sweep uses
            s += (double)ent_w[e * ld + c] / (1.0 + exp(-a));
        }
    W.pc[(size_t)blockIdx.x * 4 * LP + c] = s;
}

// candidate j: its rows of the splits, added in split order, plus the part the sweep left out -- sigma(a_j) sum_b X_b with
// sum_b X_b = B beta_out (a batch norm's output sums to its beta), and B sigma(a_j) for the bias -- into the scratch row of entity
// s_j (a label may have been there).  Without an output batch norm (!BN_OUT) sum_b X_b has no closed form: x_sum holds it in fp64.
template <bool BN_OUT>
__global__ __launch_bounds__(LP) void reduce_cand_kernel(Bufs W, const int32_t *__restrict__ sampled, const float *__restrict__ logq,
                                                         const float *__restrict__ ent_b, const float *__restrict__ beta_out,
                                                         const double *__restrict__ x_sum, int n_pos,
                                                         int n_s, int rows_p, int n_split, int dim, int ld) {
    const int j = blockIdx.x, c = threadIdx.x;
    const int64_t s = sampled[j];
    const double sig = (double)n_pos / (1.0 + exp(-(double)(ent_b[s] - logq[j])));
    if (c < dim) {
        double g = 0.0;
        for (int k = 0; k < n_split; ++k) g += (double)W.pb[((size_t)k * rows_p + j) * LP + c];
        oea::grad_add(W.s_w + s * ld + c, (float)(g + (BN_OUT ? sig * (double)beta_out[c] : sig / (double)n_pos * x_sum[c])));
    }
    if (c == 0) {
        double g = 0.0;
        for (int k = 0; k < n_split; ++k) g += (double)W.rowsum[(size_t)k * rows_p + j];
        oea::grad_add(W.s_b + s, (float)(g + sig));
    }
}

// scratch rows -> the dense fp32 gradients (read only: the scratch is cleared by the next gradient phase)
__device__ __forceinline__ void copy_row(float *g, const grad_t *s, int64_t row, int ld, int lane) {
    for (int c = lane; c < ld; c += 64) g[row * ld + c] = oea::grad_val(s[row * ld + c]);
}
__global__ __launch_bounds__(256) void convert_kernel(Bufs W, int ld, int n_pos, int n_s) {
    const int lane = threadIdx.x & 63;
    const int64_t cap = max(n_pos, n_s);
    for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < cap; i += (int64_t)gridDim.x * 4) {
        if (i < n_pos) {
            copy_row(W.g_ent, W.s_ent, W.last_h[i], ld, lane);
            copy_row(W.g_rel, W.s_rel, W.last_r[i], ld, lane);
            const int64_t t = W.last_t[i];
            copy_row(W.g_w, W.s_w, t, ld, lane);
            if (lane == 0) W.g_b[t] = oea::grad_val(W.s_b[t]);
        }
        if (i < n_s) {
            const int64_t s = W.last_s[i];
            copy_row(W.g_w, W.s_w, s, ld, lane);
            if (lane == 0) W.g_b[s] = oea::grad_val(W.s_b[s]);
        }
    }
}

// loss_accum += the label blocks, then the sweep's workgroups, each list in index order
__global__ __launch_bounds__(64) void loss_kernel(const double *__restrict__ a, int na, const double *__restrict__ b, int nb,
                                                  double *loss_accum) {
    const int lane = threadIdx.x;
    double s = 0.0;
    for (int i = lane; i < na; i += 64) s += a[i];
    for (int i = lane; i < nb; i += 64) s += b[i];
    s = oea::wave_sum_d(s);
    if (lane == 0) *loss_accum += s;
}

template <bool CF>
static void launch_sweep(int nt, dim3 grid, hipStream_t st, const SweepArgs &A) {
    switch (nt) {
        case 1: nce_sweep_kernel<CF, 1><<<grid, 64, 0, st>>>(A); break;
        case 2: nce_sweep_kernel<CF, 2><<<grid, 64, 0, st>>>(A); break;
        case 3: nce_sweep_kernel<CF, 3><<<grid, 64, 0, st>>>(A); break;
        default: nce_sweep_kernel<CF, 4><<<grid, 64, 0, st>>>(A); break;
    }
}

}  // namespace
