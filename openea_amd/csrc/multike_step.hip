// multike_step.hip -- the steps of MultiKE (approaches/multi_ke.py of the reference).
//
// 1. The attribute CNN (multi_ke.py:154-176).  For a batch of B positives (e, a, v), with the raw attribute row a, the constant
//    literal row v, the normalised entity row h and c = 1 / sqrt(1 + 1e-3):
//      x[0] = a gamma c + beta,  x[1] = v gamma c + beta                      batch norm over the width axis in inference mode
//      z1 = tanh(conv(x, K1[2,4,1,2]) + b1),  z2 = tanh(conv(z1, K2[2,4,2,2]) + b2)
//                                                       'same', cross-correlation, rows padded (0, 1), columns (1, 2)
//      n  = z2 / max(|z2| along the width, 1e-6)       per (row, channel)
//      t  = tanh(flat(n) . W[4d, d] + bd)              flat order (row, column, channel)
//      y  = t / max(|t|_F over the WHOLE [B, d] block, 1e-6)
//      loss = factor sum_b w_b softplus(|h_b - y_b|^2)
//    One or two nets with their own eight parameters share (a, v) and run as a grid dimension.  Kernels per call:
//      front    wave per batch row: batch norm, both convolutions and the width norms in LDS; stores z1, z2, the norms and flat
//      dense    32 rows per workgroup, one wave per 32 output columns on v_mfma_f32_32x32x2_f32, W from L2 into the B operand
//      loss     wave per row: y, h, the loss, dL/dh into the net's entity scratch, g = dL/dy, and <g, y>
//      dpre     dt = (g - y <g, y>_F) / |t|_F,  dpre = dt (1 - t^2), the column sums for bd
//      dflat    dpre . W^T on the matrix cores;  dW = flat^T dpre is oea_gemm_tn_f32
//      back     wave per row: back through the norms and both convolutions; da into the attribute scratch
//    Everything summed over the batch (|t|_F^2, <g, y>_F, the loss, the 52 convolution numbers, gamma, beta, bd) is an fp64 partial
//    per workgroup, added in a fixed order: the parameter gradients have the same bits in every run and in both builds.
//    Rows that repeat (entities, attributes) are summed in the step engine's scratch, whose apply phase takes them through the
//    table normalisation into the optimiser.
//
// 2. The row-wise terms of the other views (multi_ke.py:294-300, 520-527, 552, 625-638), one wave per item, one kernel:
//      CROSS    |A_h + r - B_t|^2                         two entity tables, gradients to both and to the relation row
//      PULL     coef |A_e - B_e|^2                        B constant (names) or trained (another view: its gradient too)
//      WSOFT    coef w[r] softplus(|h + r - t|^2)         the weighted positive of the predicate-aligned relation triples
#include "common.h"
#include "row_ops.h"

#include <algorithm>
#include <math.h>

namespace {

using oea::flag_t;
using oea::grad_t;

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kMaxDim = 128;
constexpr int LP = 128;               // row stride of the [B, d] buffers
constexpr int FS = 512;               // row stride of the [B, 4d] buffers
constexpr int XP = 132;               // LDS stride of a padded image row: column j lies at j + 2, j in [-2, d + 1]
constexpr int LDT = 132;              // LDS stride of the dpre tile
constexpr float kBnC = 0.99950037f;   // 1 / sqrt(1 + 1e-3)
constexpr int kRowsPerWave = 8;       // 4 waves x 8 = 32 batch rows per workgroup in every kernel
constexpr int kConvSums = 52;         // K1 16, b1 2, K2 32, b2 2
constexpr int kConvSlots = 64;
constexpr int kMaxNets = 2;
constexpr int kGradFloats = 3 * LP + kConvSlots + FS * LP;

struct Net {
    const float *gamma, *beta, *K1, *b1, *K2, *b2, *W, *bd;
    const float *ent;
    grad_t *ent_grad;
    flag_t *ent_touched;
    int weighted, l2n;
    float factor;
};

struct Bufs {
    float *z1, *z2, *flat, *df;       // [Bp, FS]
    float *t, *g;                     // [Bp, LP]
    float *nrm;                       // [Bp, 4]
    double *pt, *pq, *pl;             // [nbt]
    double *pf;                       // [nbt, kConvSlots]
    double *pg;                       // [nbt, 2, LP]
    double *pb;                       // [nbt, LP]
    double *sums;                     // [4]: |t|_F^2, <g, y>_F
    float *grads;                     // kGradFloats
};

struct Args {
    Net net[kMaxNets];
    Bufs buf[kMaxNets];
    const float *attr, *lit, *aw;
    grad_t *attr_grad;
    flag_t *attr_touched;
    const int32_t *batch;
    int n, dim, ld, nbt;
};

// the gradient block of a net: gamma, beta, bd (LP floats each), the 52 convolution numbers in the order of ConvW, W [4 dim, ld]
__host__ __device__ __forceinline__ float *g_gamma(float *g) { return g; }
__host__ __device__ __forceinline__ float *g_beta(float *g) { return g + LP; }
__host__ __device__ __forceinline__ float *g_bd(float *g) { return g + 2 * LP; }
__host__ __device__ __forceinline__ float *g_conv(float *g) { return g + 3 * LP; }
__host__ __device__ __forceinline__ float *g_w(float *g) { return g + 3 * LP + kConvSlots; }
// the eight gradients in the order of oea_multike_net.p
static void grad_pointers(float *g, float **out) {
    float *c = g_conv(g);
    float *p[8] = {g_gamma(g), g_beta(g), c, c + 16, c + 18, c + 50, g_w(g), g_bd(g)};
    for (int i = 0; i < 8; ++i) out[i] = p[i];
}

__device__ __forceinline__ int frow(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

struct ConvW { float k1[16], b1[2], k2[32], b2[2]; };
__device__ __forceinline__ ConvW load_conv(const Net &N) {
    ConvW w;
#pragma unroll
    for (int i = 0; i < 16; ++i) w.k1[i] = N.K1[i];
#pragma unroll
    for (int i = 0; i < 32; ++i) w.k2[i] = N.K2[i];
    w.b1[0] = N.b1[0]; w.b1[1] = N.b1[1]; w.b2[0] = N.b2[0]; w.b2[1] = N.b2[1];
    return w;
}

// the four pad columns of a padded LDS row of `width` floats per column: j = -2, -1, d, d + 1
__device__ __forceinline__ void zero_pads(float *row, int dim, int width, int lane) {
    if (lane < 4 * width) {
        const int p = lane / width, o = lane - p * width;
        const int idx = p < 2 ? p : dim + p;
        row[idx * width + o] = 0.f;
    }
}

// x = in gamma c + beta of both image rows into xs[2][XP]
__device__ __forceinline__ void stage_x(float *xs, const Net &N, const float *arow, const float *vrow, int dim, int lane) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int c = lane + 64 * e;
        if (c < dim) {
            const float ga = N.gamma[c] * kBnC, be = N.beta[c];
            xs[c + 2] = arow[c] * ga + be;
            xs[XP + c + 2] = vrow[c] * ga + be;
        }
    }
}

// fixed-order block sum of one double per wave -> thread 0 holds the total
__device__ __forceinline__ double block_sum4(double v, int lane, int wave, double *red) {
    v = oea::wave_sum_d(v);
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- front ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mk_front_kernel(Args A) {
    __shared__ float xs[4][2 * XP];
    __shared__ float z1s[4][2 * XP * 2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Net &N = A.net[blockIdx.y];
    const Bufs &U = A.buf[blockIdx.y];
    const int dim = A.dim;
    const ConvW w = load_conv(N);
    zero_pads(xs[wave], dim, 1, lane); zero_pads(xs[wave] + XP, dim, 1, lane);
    zero_pads(z1s[wave], dim, 2, lane); zero_pads(z1s[wave] + 2 * XP, dim, 2, lane);
    for (int r = 0; r < kRowsPerWave; ++r) {
        const int b = blockIdx.x * 32 + wave * kRowsPerWave + r;
        if (b >= A.n) break;
        const int64_t a_id = A.batch[3 * b + 1], v_id = A.batch[3 * b + 2];
        __builtin_amdgcn_wave_barrier();
        stage_x(xs[wave], N, A.attr + a_id * A.ld, A.lit + v_id * A.ld, dim, lane);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int c = lane + 64 * e;
            if (c >= dim) continue;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int o = 0; o < 2; ++o) {
                    float acc = w.b1[o];
#pragma unroll
                    for (int kh = 0; kh + i < 2; ++kh)
#pragma unroll
                        for (int kw = 0; kw < 4; ++kw) acc += xs[wave][(i + kh) * XP + c + kw + 1] * w.k1[(kh * 4 + kw) * 2 + o];
                    const float z = tanhf(acc);
                    z1s[wave][((i * XP) + c + 2) * 2 + o] = z;
                    U.z1[(size_t)b * FS + (i * dim + c) * 2 + o] = z;
                }
        }
        __builtin_amdgcn_wave_barrier();
        float z2[2][2][2], ss[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int c = lane + 64 * e;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int o = 0; o < 2; ++o) {
                    float z = 0.f;
                    if (c < dim) {
                        float acc = w.b2[o];
#pragma unroll
                        for (int kh = 0; kh + i < 2; ++kh)
#pragma unroll
                            for (int kw = 0; kw < 4; ++kw)
#pragma unroll
                                for (int ci = 0; ci < 2; ++ci)
                                    acc += z1s[wave][(((i + kh) * XP) + c + kw + 1) * 2 + ci] * w.k2[((kh * 4 + kw) * 2 + ci) * 2 + o];
                        z = tanhf(acc);
                    }
                    z2[e][i][o] = z;
                    ss[i][o] += z * z;
                }
        }
        float nr[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int o = 0; o < 2; ++o) nr[i][o] = fmaxf(sqrtf(oea::group_sum<64>(ss[i][o])), 1e-6f);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int c = lane + 64 * e;
            if (c >= dim) continue;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int o = 0; o < 2; ++o) {
                    const size_t at = (size_t)b * FS + (i * dim + c) * 2 + o;
                    U.z2[at] = z2[e][i][o];
                    U.flat[at] = z2[e][i][o] / nr[i][o];
                }
        }
        if (lane < 4) U.nrm[(size_t)b * 4 + lane] = lane == 0 ? nr[0][0] : lane == 1 ? nr[0][1] : lane == 2 ? nr[1][0] : nr[1][1];
    }
}

// ---- dense: t = tanh(flat . W + bd), the workgroup's part of |t|_F^2 -----------------------------------------------------------------
__global__ __launch_bounds__(256) void mk_dense_kernel(Args A) {
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l32 = lane & 31;
    const Net &N = A.net[blockIdx.y];
    const Bufs &U = A.buf[blockIdx.y];
    const int dim = A.dim, K4 = 4 * dim, k8 = (K4 + 7) & ~7;
    const int b0 = blockIdx.x * 32, col = 32 * wave + l32;
    const bool col_on = col < dim, row_on = b0 + l32 < A.n;
    double local = 0.0;
    if (32 * wave < dim) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const float *arow = U.flat + (size_t)(b0 + l32) * FS;
        const float *wcol = N.W + col;
        for (int q = 0; q < k8; q += 8) {
            const int k = q + 4 * half;
            const float4 a = (row_on && k < K4) ? oea::ld4(arow + k) : make_float4(0.f, 0.f, 0.f, 0.f);   // K4 % 4 == 0
            float bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) bv[i] = (col_on && k + i < K4) ? wcol[(size_t)(k + i) * A.ld] : 0.f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bv[0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bv[1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bv[2], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bv[3], acc, 0, 0, 0);
        }
        const float bias = col_on ? N.bd[col] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = b0 + frow(r, half);
            if (row < A.n && col_on) {
                const float t = tanhf(acc[r] + bias);
                U.t[(size_t)row * LP + col] = t;
                local += (double)t * (double)t;
            }
        }
    }
    const double s = block_sum4(local, lane, wave, red);
    if (threadIdx.x == 0) U.pt[blockIdx.x] = s;
}

// sums[which] of net blockIdx.x = the nbt partials in a fixed order: thread i takes i, i + 256, ..., then the threads in order
__global__ __launch_bounds__(256) void mk_reduce_kernel(Args A, int which) {
    __shared__ double red[256];
    const Bufs &U = A.buf[blockIdx.x];
    const double *p = which == 0 ? U.pt : U.pq;
    double s = 0.0;
    for (int i = threadIdx.x; i < A.nbt; i += 256) s += p[i];
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int i = 0; i < 256; ++i) tot += red[i];
        U.sums[which] = tot;
    }
}

// ---- loss: wave per row ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mk_loss_kernel(Args A) {
    __shared__ double red[4], red2[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Net &N = A.net[blockIdx.y];
    const Bufs &U = A.buf[blockIdx.y];
    const int dim = A.dim;
    const float inv_t = 1.f / fmaxf((float)sqrt(U.sums[0]), 1e-6f);
    double loss_local = 0.0, q_local = 0.0;
    for (int r = 0; r < kRowsPerWave; ++r) {
        const int b = blockIdx.x * 32 + wave * kRowsPerWave + r;
        if (b >= A.n) break;
        const int64_t e_id = A.batch[3 * b], a_id = A.batch[3 * b + 1];
        const float wgt = N.factor * (N.weighted ? A.aw[a_id] : 1.f);
        const float *hrow = N.ent + e_id * A.ld;
        float h[2], y[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int c = lane + 64 * e;
            h[e] = c < dim ? hrow[c] : 0.f;
            y[e] = c < dim ? U.t[(size_t)b * LP + c] * inv_t : 0.f;
        }
        const float inv = N.l2n ? rsqrtf(fmaxf(oea::group_sum<64>(h[0] * h[0] + h[1] * h[1]), 1e-12f)) : 1.f;
        const float d0 = h[0] * inv - y[0], d1 = h[1] * inv - y[1];
        const float dist = oea::group_sum<64>(d0 * d0 + d1 * d1);
        const float s2 = 2.f * wgt * oea::row::sigmoid_f(dist);
        loss_local += (double)wgt * (double)oea::row::softplus_f(dist);
        const float g0 = -s2 * d0, g1 = -s2 * d1;        // dL/dy; dL/dh is its negative
        q_local += (double)oea::group_sum<64>(g0 * y[0] + g1 * y[1]);
        grad_t *dst = N.ent_grad + e_id * A.ld;
        if (lane < dim) { oea::grad_add(dst + lane, -g0); U.g[(size_t)b * LP + lane] = g0; }
        if (lane + 64 < dim) { oea::grad_add(dst + lane + 64, -g1); U.g[(size_t)b * LP + lane + 64] = g1; }
        if (lane == 0) N.ent_touched[e_id] = 1;
    }
    if (lane == 0) { red[wave] = loss_local; red2[wave] = q_local; }       // every lane holds its wave's sums
    __syncthreads();
    if (threadIdx.x == 0) {
        U.pl[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
        U.pq[blockIdx.x] = (red2[0] + red2[1]) + (red2[2] + red2[3]);
    }
}

// ---- dpre: thread = column, block = 32 rows ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(LP) void mk_dpre_kernel(Args A) {
    const Bufs &U = A.buf[blockIdx.y];
    const int c = threadIdx.x, b0 = blockIdx.x * 32;
    const float tn = (float)sqrt(U.sums[0]), sq = (float)U.sums[1];
    const bool clamped = tn < 1e-6f;
    const float inv_t = 1.f / fmaxf(tn, 1e-6f);
    double s = 0.0;
    for (int b = b0; b < b0 + 32; ++b) {
        float dp = 0.f;
        if (b < A.n && c < A.dim) {
            const float t = U.t[(size_t)b * LP + c], g = U.g[(size_t)b * LP + c];
            const float dt = clamped ? g * inv_t : (g - (t * inv_t) * sq) * inv_t;
            dp = dt * (1.f - t * t);
        }
        U.g[(size_t)b * LP + c] = dp;
        s += (double)dp;
    }
    U.pb[(size_t)blockIdx.x * LP + c] = s;
}

// ---- dflat = dpre . W^T ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mk_dflat_kernel(Args A) {
    __shared__ __attribute__((aligned(16))) float Zs[32 * LDT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l32 = lane & 31;
    const Net &N = A.net[blockIdx.y];
    const Bufs &U = A.buf[blockIdx.y];
    const int dim = A.dim, K4 = 4 * dim, kd8 = (dim + 7) & ~7;
    const int b0 = blockIdx.x * 32;
    for (int idx = threadIdx.x; idx < 32 * 32; idx += 256) {
        const int row = idx >> 5, c4 = (idx & 31) * 4;
        oea::st4(Zs + row * LDT + c4, oea::ld4(U.g + (size_t)(b0 + row) * LP + c4));      // rows >= n and columns >= dim hold zeros
    }
    __syncthreads();
    for (int ct = wave; 32 * ct < K4; ct += 4) {
        const int kk = 32 * ct + l32;
        const bool valid = kk < K4;
        const float *wrow = N.W + (size_t)(valid ? kk : 0) * A.ld;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int q = 0; q < kd8; q += 8) {
            const int nn = q + 4 * half;
            const float4 a = oea::ld4(Zs + l32 * LDT + nn);
            const float4 bq = (valid && nn < A.ld) ? oea::ld4(wrow + nn) : make_float4(0.f, 0.f, 0.f, 0.f);   // ld % 4 == 0
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bq.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bq.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bq.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bq.w, acc, 0, 0, 0);
        }
        if (valid)
#pragma unroll
            for (int r = 0; r < 16; ++r) U.df[(size_t)(b0 + frow(r, half)) * FS + kk] = acc[r];
    }
}

// ---- back: wave per row -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mk_back_kernel(Args A) {
    __shared__ float xs[4][2 * XP];
    __shared__ float z1s[4][2 * XP * 2], dp2s[4][2 * XP * 2], dp1s[4][2 * XP * 2];
    __shared__ double red[4][kConvSums];
    __shared__ double redg[4][2][LP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Net &N = A.net[blockIdx.y];
    const Bufs &U = A.buf[blockIdx.y];
    const int dim = A.dim;
    const ConvW w = load_conv(N);
    float sm[kConvSums];
#pragma unroll
    for (int i = 0; i < kConvSums; ++i) sm[i] = 0.f;
    float gga[2] = {0.f, 0.f}, gbe[2] = {0.f, 0.f};
    zero_pads(xs[wave], dim, 1, lane); zero_pads(xs[wave] + XP, dim, 1, lane);
    zero_pads(z1s[wave], dim, 2, lane); zero_pads(z1s[wave] + 2 * XP, dim, 2, lane);
    zero_pads(dp2s[wave], dim, 2, lane); zero_pads(dp2s[wave] + 2 * XP, dim, 2, lane);
    zero_pads(dp1s[wave], dim, 2, lane); zero_pads(dp1s[wave] + 2 * XP, dim, 2, lane);
    for (int r = 0; r < kRowsPerWave; ++r) {
        const int b = blockIdx.x * 32 + wave * kRowsPerWave + r;
        if (b >= A.n) break;
        const int64_t a_id = A.batch[3 * b + 1], v_id = A.batch[3 * b + 2];
        const float *arow = A.attr + a_id * A.ld, *vrow = A.lit + v_id * A.ld;
        __builtin_amdgcn_wave_barrier();
        stage_x(xs[wave], N, arow, vrow, dim, lane);
        // through the width normalisation
        float dn[2][2][2], nv[2][2][2], z2[2][2][2], pr[2][2] = {{0.f, 0.f}, {0.f, 0.f}}, nr[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int o = 0; o < 2; ++o) nr[i][o] = U.nrm[(size_t)b * 4 + i * 2 + o];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int c = lane + 64 * e;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int o = 0; o < 2; ++o) {
                    const size_t at = (size_t)b * FS + (i * dim + c) * 2 + o;
                    const bool on = c < dim;
                    dn[e][i][o] = on ? U.df[at] : 0.f;
                    z2[e][i][o] = on ? U.z2[at] : 0.f;
                    nv[e][i][o] = z2[e][i][o] / nr[i][o];
                    pr[i][o] += dn[e][i][o] * nv[e][i][o];
                    if (on) z1s[wave][((i * XP) + c + 2) * 2 + o] = U.z1[at];
                }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int o = 0; o < 2; ++o) pr[i][o] = nr[i][o] <= 1e-6f ? 0.f : oea::group_sum<64>(pr[i][o]);   // clamped: n = z2 / 1e-6
        float dp2[2][2][2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int c = lane + 64 * e;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int o = 0; o < 2; ++o) {
                    const float dz = (dn[e][i][o] - nv[e][i][o] * pr[i][o]) / nr[i][o];
                    const float v = dz * (1.f - z2[e][i][o] * z2[e][i][o]);
                    dp2[e][i][o] = v;
                    sm[50 + o] += v;
                    if (c < dim) dp2s[wave][((i * XP) + c + 2) * 2 + o] = v;
                }
        }
        __builtin_amdgcn_wave_barrier();
        // dK2, then dz1 -> dp1
        float dp1[2][2][2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int c = lane + 64 * e;
            if (c >= dim) {
#pragma unroll
                for (int i = 0; i < 2; ++i) { dp1[e][i][0] = 0.f; dp1[e][i][1] = 0.f; }
                continue;
            }
#pragma unroll
            for (int kh = 0; kh < 2; ++kh)
#pragma unroll
                for (int kw = 0; kw < 4; ++kw)
#pragma unroll
                    for (int ci = 0; ci < 2; ++ci)
#pragma unroll
                        for (int i = 0; i + kh < 2; ++i) {
                            const float zin = z1s[wave][(((i + kh) * XP) + c + kw + 1) * 2 + ci];
                            sm[18 + ((kh * 4 + kw) * 2 + ci) * 2 + 0] += dp2[e][i][0] * zin;
                            sm[18 + ((kh * 4 + kw) * 2 + ci) * 2 + 1] += dp2[e][i][1] * zin;
                        }
#pragma unroll
            for (int ip = 0; ip < 2; ++ip)
#pragma unroll
                for (int ci = 0; ci < 2; ++ci) {
                    float acc = 0.f;
#pragma unroll
                    for (int kh = 0; kh <= ip; ++kh)
#pragma unroll
                        for (int kw = 0; kw < 4; ++kw)
#pragma unroll
                            for (int o = 0; o < 2; ++o)
                                acc += dp2s[wave][(((ip - kh) * XP) + c - kw + 3) * 2 + o] * w.k2[((kh * 4 + kw) * 2 + ci) * 2 + o];
                    const float z = z1s[wave][((ip * XP) + c + 2) * 2 + ci];
                    const float v = acc * (1.f - z * z);
                    dp1[e][ip][ci] = v;
                    sm[16 + ci] += v;
                    dp1s[wave][((ip * XP) + c + 2) * 2 + ci] = v;
                }
        }
        __builtin_amdgcn_wave_barrier();
        // dK1, then dx -> gamma, beta, the attribute row
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int c = lane + 64 * e;
            if (c >= dim) continue;
#pragma unroll
            for (int kh = 0; kh < 2; ++kh)
#pragma unroll
                for (int kw = 0; kw < 4; ++kw)
#pragma unroll
                    for (int i = 0; i + kh < 2; ++i) {
                        const float xin = xs[wave][(i + kh) * XP + c + kw + 1];
                        sm[(kh * 4 + kw) * 2 + 0] += dp1[e][i][0] * xin;
                        sm[(kh * 4 + kw) * 2 + 1] += dp1[e][i][1] * xin;
                    }
            float dx[2];
#pragma unroll
            for (int ip = 0; ip < 2; ++ip) {
                float acc = 0.f;
#pragma unroll
                for (int kh = 0; kh <= ip; ++kh)
#pragma unroll
                    for (int kw = 0; kw < 4; ++kw)
#pragma unroll
                        for (int o = 0; o < 2; ++o) acc += dp1s[wave][(((ip - kh) * XP) + c - kw + 3) * 2 + o] * w.k1[(kh * 4 + kw) * 2 + o];
                dx[ip] = acc;
            }
            gga[e] += (dx[0] * arow[c] + dx[1] * vrow[c]) * kBnC;
            gbe[e] += dx[0] + dx[1];
            oea::grad_add(A.attr_grad + a_id * A.ld + c, dx[0] * (N.gamma[c] * kBnC));
        }
        if (lane == 0) A.attr_touched[a_id] = 1;
    }
#pragma unroll
    for (int i = 0; i < kConvSums; ++i) {
        const double t = oea::wave_sum_d((double)sm[i]);
        if (lane == 0) red[wave][i] = t;
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        redg[wave][0][lane + 64 * e] = (double)gga[e];
        redg[wave][1][lane + 64 * e] = (double)gbe[e];
    }
    __syncthreads();
    if (threadIdx.x < kConvSums)
        U.pf[(size_t)blockIdx.x * kConvSlots + threadIdx.x] =
            (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    {
        const int which = threadIdx.x >> 7, c = threadIdx.x & 127;
        U.pg[((size_t)blockIdx.x * 2 + which) * LP + c] = (redg[0][which][c] + redg[1][which][c]) + (redg[2][which][c] + redg[3][which][c]);
    }
}

// the small gradients out of the partials: every column's partials in four quarters of the workgroups, each added in workgroup order
// by its own thread, the quarters then in order; block 0 adds the loss of every net, net after net
constexpr int kSmallCols = 64 + LP;
__global__ __launch_bounds__(4 * kSmallCols) void mk_small_kernel(Args A, int n_nets, double *loss_accum) {
    __shared__ double part[4][3][kSmallCols];
    const Bufs &U = A.buf[blockIdx.x];
    const int q = threadIdx.x / kSmallCols, t = threadIdx.x - q * kSmallCols;
    const int b0 = (int)((int64_t)q * A.nbt / 4), b1 = (int)((int64_t)(q + 1) * A.nbt / 4);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    if (t < kConvSums) {
        for (int b = b0; b < b1; ++b) s0 += U.pf[(size_t)b * kConvSlots + t];
    } else if (t >= 64) {
        const int c = t - 64;
        for (int b = b0; b < b1; ++b) {
            s0 += U.pg[((size_t)b * 2) * LP + c]; s1 += U.pg[((size_t)b * 2 + 1) * LP + c]; s2 += U.pb[(size_t)b * LP + c];
        }
    } else if (blockIdx.x == 0 && t == 63) {
        for (int k = 0; k < n_nets; ++k)
            for (int b = b0; b < b1; ++b) s0 += A.buf[k].pl[b];
    }
    part[q][0][t] = s0; part[q][1][t] = s1; part[q][2][t] = s2;
    __syncthreads();
    if (q != 0) return;
    double r[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) r[i] = (part[0][i][t] + part[1][i][t]) + (part[2][i][t] + part[3][i][t]);
    if (t < kConvSums) g_conv(U.grads)[t] = (float)r[0];
    else if (t >= 64) {
        g_gamma(U.grads)[t - 64] = (float)r[0]; g_beta(U.grads)[t - 64] = (float)r[1]; g_bd(U.grads)[t - 64] = (float)r[2];
    } else if (blockIdx.x == 0 && t == 63) atomicAdd(loss_accum, r[0]);
}

// SGD on the eight parameters of every net in one launch: blockIdx.y = parameter, blockIdx.z = net
struct SgdArgs {
    float *p[kMaxNets][8];
    const float *g[kMaxNets][8];
    int64_t n[8];
    float lr;
};
__global__ __launch_bounds__(256) void mk_sgd_kernel(SgdArgs S) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < S.n[blockIdx.y]) S.p[blockIdx.z][blockIdx.y][i] -= S.lr * S.g[blockIdx.z][blockIdx.y][i];
}

// ---- workspace ------------------------------------------------------------------------------------------------------------------
struct Layout {
    size_t z1, z2, flat, df, t, g, nrm, pt, pq, pl, pf, pg, pb, sums, grads, per_net, gemm, total;
    int nbt;
};

static Layout make_layout(int64_t max_n, int32_t dim, int32_t ld) {
    Layout L;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += oea::align256(bytes); return at; };
    L.nbt = (int)std::max<int64_t>(1, (max_n + 31) / 32);
    const size_t Bp = (size_t)L.nbt * 32, nb = (size_t)L.nbt;
    L.z1 = take(4 * Bp * FS); L.z2 = take(4 * Bp * FS); L.flat = take(4 * Bp * FS); L.df = take(4 * Bp * FS);
    L.t = take(4 * Bp * LP); L.g = take(4 * Bp * LP); L.nrm = take(4 * Bp * 4);
    L.pt = take(8 * nb); L.pq = take(8 * nb); L.pl = take(8 * nb);
    L.pf = take(8 * nb * kConvSlots); L.pg = take(8 * nb * 2 * LP); L.pb = take(8 * nb * LP);
    L.sums = take(8 * 4); L.grads = take(4 * (size_t)kGradFloats);
    L.per_net = o;
    L.gemm = kMaxNets * L.per_net;
    L.total = L.gemm + oea::align256(4 * std::max<size_t>(1, oea_gemm_tn_workspace_floats(max_n, 4 * dim, ld)));
    return L;
}

static Bufs bufs_of(void *ws, const Layout &L, int net) {
    char *b = static_cast<char *>(ws) + (size_t)net * L.per_net;
    Bufs U;
    U.z1 = (float *)(b + L.z1); U.z2 = (float *)(b + L.z2); U.flat = (float *)(b + L.flat); U.df = (float *)(b + L.df);
    U.t = (float *)(b + L.t); U.g = (float *)(b + L.g); U.nrm = (float *)(b + L.nrm);
    U.pt = (double *)(b + L.pt); U.pq = (double *)(b + L.pq); U.pl = (double *)(b + L.pl);
    U.pf = (double *)(b + L.pf); U.pg = (double *)(b + L.pg); U.pb = (double *)(b + L.pb);
    U.sums = (double *)(b + L.sums); U.grads = (float *)(b + L.grads);
    return U;
}

static int check_shape(const char *who, int32_t dim, int32_t ld, int64_t max_n) {
    if (!(ld % 4 == 0 && dim > 0 && dim <= ld && max_n >= 1 && max_n < (1LL << 24))) {
        oea::set_error("%s: invalid argument: ld %% 4 == 0, 0 < dim <= ld, 1 <= max_n < 2^24", who);
        return OEA_EINVAL;
    }
    if (dim > kMaxDim) { oea::set_error("%s: dim %d > %d", who, dim, kMaxDim); return OEA_EUNSUPPORTED; }
    return OEA_OK;
}

// ---- the row-wise terms ------------------------------------------------------------------------------------------------------------
constexpr int kRowWaves = 4;
constexpr int kRowMaxBlocks = 2048;

struct RowArgs {
    int kind;
    const float *ta, *tb, *rel, *w;
    int a_l2n, b_l2n, rel_l2n, b_trained;
    grad_t *ga, *gb, *gr;
    flag_t *fa, *fb, *fr;
    const int32_t *items;
    int64_t n;
    int ld, dim;
    float coef;
    double *loss_accum;
};

__device__ __forceinline__ void add_row(grad_t *grad, flag_t *touched, int64_t row, int ld, int dim, int lane, float g0, float g1) {
    grad_t *p = grad + row * ld;
    if (lane < dim) oea::grad_add(p + lane, g0);
    if (lane + 64 < dim) oea::grad_add(p + lane + 64, g1);
    if (lane == 0) touched[row] = 1;
}

struct Row2 { float v0, v1; };
__device__ __forceinline__ Row2 unit_row(const float *table, int64_t row, int ld, int dim, int lane, int l2n) {
    const float *p = table + row * ld;
    Row2 r;
    r.v0 = lane < dim ? p[lane] : 0.f;
    r.v1 = lane + 64 < dim ? p[lane + 64] : 0.f;
    if (l2n) {
        const float inv = rsqrtf(fmaxf(oea::group_sum<64>(r.v0 * r.v0 + r.v1 * r.v1), 1e-12f));
        r.v0 *= inv; r.v1 *= inv;
    }
    return r;
}

__global__ __launch_bounds__(64 * kRowWaves) void mk_rows_kernel(RowArgs A) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double loss_local = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * kRowWaves + wave; p < A.n; p += (int64_t)gridDim.x * kRowWaves) {
        if (A.kind == OEA_MULTIKE_ROWS_PULL) {
            const int64_t e = A.items[p];
            const Row2 a = unit_row(A.ta, e, A.ld, A.dim, lane, A.a_l2n), b = unit_row(A.tb, e, A.ld, A.dim, lane, A.b_l2n);
            const float d0 = a.v0 - b.v0, d1 = a.v1 - b.v1;
            loss_local += (double)A.coef * (double)oea::group_sum<64>(d0 * d0 + d1 * d1);
            const float c2 = 2.f * A.coef;
            add_row(A.ga, A.fa, e, A.ld, A.dim, lane, c2 * d0, c2 * d1);
            if (A.b_trained) add_row(A.gb, A.fb, e, A.ld, A.dim, lane, -c2 * d0, -c2 * d1);
        } else {
            const int64_t h = A.items[3 * p], r = A.items[3 * p + 1], t = A.items[3 * p + 2];
            const Row2 a = unit_row(A.ta, h, A.ld, A.dim, lane, A.a_l2n), b = unit_row(A.tb, t, A.ld, A.dim, lane, A.b_l2n);
            const Row2 u = unit_row(A.rel, r, A.ld, A.dim, lane, A.rel_l2n);
            const float d0 = a.v0 + u.v0 - b.v0, d1 = a.v1 + u.v1 - b.v1;
            const float dist = oea::group_sum<64>(d0 * d0 + d1 * d1);
            float c2;
            if (A.kind == OEA_MULTIKE_ROWS_WSOFT) {
                const float wgt = A.coef * A.w[r];
                loss_local += (double)wgt * (double)oea::row::softplus_f(dist);
                c2 = 2.f * wgt * oea::row::sigmoid_f(dist);
            } else {
                loss_local += (double)A.coef * (double)dist;
                c2 = 2.f * A.coef;
            }
            add_row(A.ga, A.fa, h, A.ld, A.dim, lane, c2 * d0, c2 * d1);
            add_row(A.gb, A.fb, t, A.ld, A.dim, lane, -c2 * d0, -c2 * d1);
            add_row(A.gr, A.fr, r, A.ld, A.dim, lane, c2 * d0, c2 * d1);
        }
    }
    oea::block_loss_add<kRowWaves>(loss_local, lane, wave, A.loss_accum);
}

}  // namespace

extern "C" {

size_t oea_multike_cnn_workspace_bytes(int32_t dim, int32_t ld, int64_t max_n) {
    if (check_shape("oea_multike_cnn_workspace_bytes", dim, ld, max_n) != OEA_OK) return 0;
    return make_layout(max_n, dim, ld).total;
}

int oea_multike_cnn_grads(void *workspace, int32_t dim, int32_t ld, int64_t max_n, int32_t net, void **grads) {
    const int rc = check_shape("oea_multike_cnn_grads", dim, ld, max_n);
    if (rc != OEA_OK) return rc;
    OEA_REQUIRE(workspace && grads && net >= 0 && net < kMaxNets, "workspace / grads / net");
    const Bufs U = bufs_of(workspace, make_layout(max_n, dim, ld), net);
    float *out[8];
    grad_pointers(U.grads, out);
    for (int i = 0; i < 8; ++i) grads[i] = out[i];
    return OEA_OK;
}

int oea_multike_cnn_step(const oea_multike_net *nets, int32_t n_nets, int64_t n_ent, const float *attr, int64_t n_attr,
                         const float *lit, int64_t n_lit, int32_t dim, int32_t ld, const int32_t *batch, int64_t n,
                         const float *attr_weight, float lr, void *workspace, int64_t max_n, double *loss_accum, int32_t phase,
                         void *stream) {
    OEA_REQUIRE(nets && attr && lit && workspace && loss_accum, "null pointer");
    OEA_REQUIRE(n_nets >= 1 && n_nets <= kMaxNets, "1 or 2 nets");
    OEA_REQUIRE(phase == OEA_PHASE_BOTH || phase == OEA_PHASE_GRAD, "phase: OEA_PHASE_BOTH or OEA_PHASE_GRAD (the tables apply through the engine)");
    const int rc = check_shape("oea_multike_cnn_step", dim, ld, max_n);
    if (rc != OEA_OK) return rc;
    OEA_REQUIRE(n_ent > 0 && n_attr > 0 && n_lit > 0 && n_ent < (1LL << 31), "table rows");
    OEA_REQUIRE(n >= 1 && n <= max_n && batch, "1 <= n <= max_n");
    OEA_REQUIRE(lr >= 0.f, "lr >= 0");
    for (int k = 0; k < n_nets; ++k) {
        for (int i = 0; i < 8; ++i) OEA_REQUIRE(nets[k].p[i], "null parameter");
        OEA_REQUIRE(nets[k].ent && nets[k].step_workspace && nets[k].n_rel_ws > 0, "net: entity table / step workspace");
        OEA_REQUIRE(!nets[k].weighted || attr_weight, "a weighted net needs attr_weight");
    }
    OEA_REQUIRE(nets[0].n_rel_ws == n_attr, "net 0's step workspace holds the attribute rows: n_rel_ws == n_attr");
    const Layout L = make_layout(max_n, dim, ld);
    OEA_REQUIRE(oea_gemm_tn_workspace_floats(n, 4 * dim, ld) * 4 <= L.total - L.gemm, "gemm workspace");
    hipStream_t st = oea::as_stream(stream);
    Args A;
    A.attr = attr; A.lit = lit; A.aw = attr_weight; A.batch = batch; A.n = (int)n; A.dim = dim; A.ld = ld;
    A.nbt = (int)((n + 31) / 32);
    for (int k = 0; k < kMaxNets; ++k) {
        const oea_multike_net &s = nets[k < n_nets ? k : 0];
        Net &N = A.net[k];
        N.gamma = s.p[0]; N.beta = s.p[1]; N.K1 = s.p[2]; N.b1 = s.p[3]; N.K2 = s.p[4]; N.b2 = s.p[5]; N.W = s.p[6]; N.bd = s.p[7];
        N.ent = s.ent; N.weighted = s.weighted; N.l2n = s.ent_l2_norm; N.factor = s.factor;
        grad_t *rg;
        flag_t *rt;
        oea::step_scratch_rows(s.step_workspace, n_ent, s.n_rel_ws, ld, &N.ent_grad, &N.ent_touched, &rg, &rt);
        if (k == 0) { A.attr_grad = rg; A.attr_touched = rt; }
        A.buf[k] = bufs_of(workspace, L, k);
    }
    const dim3 grid(A.nbt, n_nets);
    mk_front_kernel<<<grid, 256, 0, st>>>(A);
    mk_dense_kernel<<<grid, 256, 0, st>>>(A);
    mk_reduce_kernel<<<n_nets, 256, 0, st>>>(A, 0);
    mk_loss_kernel<<<grid, 256, 0, st>>>(A);
    mk_reduce_kernel<<<n_nets, 256, 0, st>>>(A, 1);
    mk_dpre_kernel<<<grid, LP, 0, st>>>(A);
    mk_dflat_kernel<<<grid, 256, 0, st>>>(A);
    mk_back_kernel<<<grid, 256, 0, st>>>(A);
    mk_small_kernel<<<n_nets, 4 * kSmallCols, 0, st>>>(A, n_nets, loss_accum);
    OEA_CHECK_HIP(hipGetLastError());
    float *gemm_ws = (float *)(static_cast<char *>(workspace) + L.gemm);
    for (int k = 0; k < n_nets; ++k) {
        const int r = oea_gemm_tn_f32(A.buf[k].flat, FS, 4 * dim, A.buf[k].g, LP, ld, n, g_w(A.buf[k].grads), ld, gemm_ws, stream);
        if (r != OEA_OK) return r;
    }
    if (phase == OEA_PHASE_BOTH) {
        const int64_t cnt[8] = {dim, dim, 16, 2, 32, 2, (int64_t)4 * dim * ld, dim};
        SgdArgs S;
        S.lr = lr;
        for (int i = 0; i < 8; ++i) S.n[i] = cnt[i];
        for (int k = 0; k < kMaxNets; ++k) {
            float *src[8];
            grad_pointers(A.buf[k < n_nets ? k : 0].grads, src);
            for (int i = 0; i < 8; ++i) { S.p[k][i] = nets[k < n_nets ? k : 0].p[i]; S.g[k][i] = src[i]; }
        }
        mk_sgd_kernel<<<dim3((unsigned)oea::ceil_div(cnt[6], 256), 8, n_nets), 256, 0, st>>>(S);
        OEA_CHECK_HIP(hipGetLastError());
    }
    return OEA_OK;
}

int oea_multike_rows(int32_t kind, const float *table_a, void *ws_a, int64_t n_rel_a, int32_t a_l2_norm, const float *table_b,
                     void *ws_b, int64_t n_rel_b, int32_t b_l2_norm, const float *rel, int32_t rel_l2_norm, int64_t n_ent,
                     int32_t rel_side, int32_t dim, int32_t ld, const int32_t *items, int64_t n, const float *rel_weight, float coef,
                     double *loss_accum, void *stream) {
    OEA_REQUIRE(rel_side == 0 || rel_side == 1, "rel_side: 0 (the relation rows lie in ws_a) or 1 (in ws_b)");
    OEA_REQUIRE(kind == OEA_MULTIKE_ROWS_CROSS || kind == OEA_MULTIKE_ROWS_PULL || kind == OEA_MULTIKE_ROWS_WSOFT, "kind");
    OEA_REQUIRE(table_a && ws_a && table_b && loss_accum && n_ent > 0 && n_rel_a > 0, "null pointer / rows");
    OEA_REQUIRE(ld % 4 == 0 && dim > 0 && dim <= ld, "ld % 4 == 0, 0 < dim <= ld");
    OEA_REQUIRE(n >= 0 && (items || n == 0), "items");
    if (dim > kMaxDim) { oea::set_error("oea_multike_rows: dim %d > %d", dim, kMaxDim); return OEA_EUNSUPPORTED; }
    if (kind != OEA_MULTIKE_ROWS_PULL) OEA_REQUIRE(rel && ws_b && n_rel_b > 0, "CROSS / WSOFT: relation table, both workspaces");
    if (kind == OEA_MULTIKE_ROWS_WSOFT) OEA_REQUIRE(rel_weight, "WSOFT: rel_weight");
    if (n == 0) return OEA_OK;
    RowArgs A;
    A.kind = kind; A.ta = table_a; A.tb = table_b; A.rel = rel; A.w = rel_weight;
    A.a_l2n = a_l2_norm; A.b_l2n = b_l2_norm; A.rel_l2n = rel_l2_norm; A.b_trained = ws_b != nullptr;
    A.items = items; A.n = n; A.ld = ld; A.dim = dim; A.coef = coef; A.loss_accum = loss_accum;
    grad_t *rg;
    flag_t *rt;
    oea::step_scratch_rows(ws_a, n_ent, n_rel_a, ld, &A.ga, &A.fa, &A.gr, &A.fr);
    A.gb = nullptr; A.fb = nullptr;
    if (ws_b) {
        oea::step_scratch_rows(ws_b, n_ent, n_rel_b, ld, &A.gb, &A.fb, &rg, &rt);
        if (rel_side == 1) { A.gr = rg; A.fr = rt; }
    }
    const unsigned grid = (unsigned)std::min<int64_t>(oea::ceil_div(n, kRowWaves), kRowMaxBlocks);
    mk_rows_kernel<<<grid, 64 * kRowWaves, 0, oea::as_stream(stream)>>>(A);
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

}  // extern "C"
