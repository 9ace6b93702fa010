// conve_step.hip -- the training step of ConvE (models/neural/conve.py:21-79 of the reference): ProjE's sampled-softmax (NCE) back
// end behind a 3 x 3 convolution and a dense layer, under TF's dense Adam.
//
//   img = [l2n(ent)[h] ; l2n(rel)[r]] as a [2x, y] image (x y = d, 2d values);   c = 1 / sqrt(1 + 1e-3)
//   s   = drop0(img o gamma1[col] c + beta1[col])
//   z1_f = conv3x3(s, kern[:, :, 0, f]) + cbias[f]   ('same', zero padding, cross-correlation)
//   a_f  = drop1(relu(z1_f gamma2[f] c + beta2[f]))                              [F, 2x, y] flattened f-major: K = 2 d F values
//   z2  = a . fcW + fcb;  X = relu(z2) o gamma3 c + beta3;  loss = nce_loss(entity_w, entity_b, t, X)  (nce_half.h)
//
// The B x K activation `a` never exists in memory.  Three kernels on v_mfma_f32_32x32x2_f32 (exact fp32 products) rebuild the tile
// of it they need in LDS, from the 2d-float rows of s: 9-tap convolution, BN2, relu, mask -- one device function, so that the three
// see the same bits.
//   forward   (batch-major)   a workgroup owns 32 batch rows and walks its share of the filters (blockIdx.y): z2 += a_f . fcW_f,
//                             wave w owns output columns 32 w .. 32 w + 31, fcW goes from L2 straight into the B operand
//   backward-data (batch-major)  per filter: da = dz2 . fcW_f^T, then mask / relu sign / gamma2 c, the filter's own gradients as
//                             fp64 block partials, and the transposed convolution into the rows' ds, accumulated over the filters
//                             in LDS by the thread that owns the element (no atomics)
//   backward-weight (filter-major)  a workgroup owns the 2d rows of fcW of one filter and walks its share of the batch tiles
//                             (blockIdx.y): dfcW_f += a_f^T . dz2
// Every split writes its own partial; the splits are added in split order.  Everything reduced over the batch goes through fp64
// block partials summed in block order.  Rows that repeat (heads, relations, labels, candidates) are summed in the step scratch's
// element type: fp32 atomics, or int64 fixed point in the deterministic build.
//
// Without an output batch norm the two parts of the NCE gradient that the sweeps leave out (nce_half.h works with sigma_bj -
// sigma(a_j)) have no closed form: the common vector sum_j sigma(a_j) W[s_j] is added to every row's dX, and dW[s_j] gets
// sigma(a_j) sum_b X_b with the batch sum reduced in fp64.
#include "nce_half.h"

#include <math.h>

namespace {

constexpr int kMaxFilters = 64;
constexpr int LP2 = 256;              // row stride of the 2d-wide batch buffers
constexpr int kFSlots = 16;           // fp64 slots per (row tile, filter): gamma2, beta2, cbias, 9 taps
constexpr int kFSums = 12;
constexpr float kBnC = 0.99950037f;   // 1 / sqrt(1 + 1e-3)
constexpr uint32_t kMaskTag = 0x436f6e00u;
constexpr int kThreads = 256;

struct Geo {
    int dim, ld, x, y, d2, k8, sp, ap, F;
    float inv_keep;
    uint32_t thr;        // an element is kept iff its 16-bit lane < thr; 65536: nothing is drawn
    uint32_t seed_lo, seed_hi, step;
};

static void factorize(int d, int *x, int *y) {
    int half = (int)sqrt((double)d) + 1;
    while (d % half > 0) --half;
    *x = half; *y = d / half;
}

// ---- workspace ---------------------------------------------------------------------------------------------------------------
struct CBufs {
    float *g_g1, *g_b1, *g_kern, *g_cb, *g_g2, *g_b2, *g_fcw, *g_fcb, *g_g3, *g_b3;
    float *img, *s, *dv;      // [B, LP2]
    float *pz, *dsp, *pw;     // the split partials: forward [split][rows][LP], ds [split][rows][LP2], dfcW [split][K][LP]
    double *pf;               // [row tiles][F][kFSlots]
};

struct CLayout {
    size_t g_ent, g_rel, g_w, g_b, s_ent, s_rel, s_w, s_b, last_h, last_r, last_t, last_s, last_n;
    size_t g_g1, g_b1, g_kern, g_cb, g_g2, g_b2, g_fcw, g_fcb, g_g3, g_b3;
    size_t z2, x, dxlab, dx, invh, invr, dtrue, p, pc, sums, pa, pb, rowsum, loss_a, loss_l;
    size_t img, s, dv, pz, dsp, pw, pf;
    size_t total;
    int nbt, nct;
};

static CLayout make_layout(int64_t n_ent, int64_t n_rel, int dim, int ld, int F, int64_t max_pos, int64_t max_s) {
    CLayout L;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += oea::align256(bytes); return at; };
    const size_t E = (size_t)n_ent, R = (size_t)n_rel, B = (size_t)max_pos, S = (size_t)max_s, K = (size_t)2 * dim * F;
    L.g_ent = take(4 * E * ld); L.g_rel = take(4 * R * ld); L.g_w = take(4 * E * ld); L.g_b = take(4 * E);
    L.g_g1 = take(4 * LP); L.g_b1 = take(4 * LP); L.g_kern = take(4 * 9 * kMaxFilters); L.g_cb = take(4 * kMaxFilters);
    L.g_g2 = take(4 * kMaxFilters); L.g_b2 = take(4 * kMaxFilters); L.g_fcw = take(4 * K * ld); L.g_fcb = take(4 * LP);
    L.g_g3 = take(4 * LP); L.g_b3 = take(4 * LP);
    L.s_ent = take(sizeof(grad_t) * E * ld); L.s_rel = take(sizeof(grad_t) * R * ld); L.s_w = take(sizeof(grad_t) * E * ld);
    L.s_b = take(sizeof(grad_t) * E);
    L.last_h = take(4 * B); L.last_r = take(4 * B); L.last_t = take(4 * B); L.last_s = take(4 * S); L.last_n = take(16);
    L.nbt = std::max(1, (int)((B + 31) / 32)); L.nct = std::max(1, (int)((S + 31) / 32));
    const size_t Bp = (size_t)L.nbt * 32;
    // a smaller batch than the capacity may be split further: split(n) n <= min(kMaxSplit n, kTargetWgs - 1 + n), monotone in n
    const size_t Ba = 32 * std::min<size_t>((size_t)kMaxSplit * L.nbt, (size_t)kTargetWgs - 1 + L.nbt);
    const size_t Sb = 32 * std::min<size_t>((size_t)kMaxSplit * L.nct, (size_t)kTargetWgs - 1 + L.nct);
    L.z2 = take(4 * Bp * LP); L.x = take(4 * Bp * LP); L.dxlab = take(4 * Bp * LP); L.dx = take(4 * Bp * LP);
    L.invh = take(4 * Bp); L.invr = take(4 * Bp); L.dtrue = take(4 * Bp);
    L.p = take(8 * (size_t)L.nbt * 4 * LP); L.pc = take(8 * (size_t)L.nct * 4 * LP); L.sums = take(8 * 5 * 4 * LP);
    L.pa = take(4 * Ba * LP); L.pb = take(4 * Sb * LP); L.rowsum = take(4 * Sb);
    L.loss_a = take(8 * Ba / 32); L.loss_l = take(8 * (B / 4 + 1));
    L.img = take(4 * Bp * LP2); L.s = take(4 * Bp * LP2); L.dv = take(4 * Bp * LP2);
    L.pz = take(4 * Ba * LP); L.dsp = take(4 * Ba * LP2);
    L.pw = take(4 * (size_t)std::min(kMaxSplit, L.nbt) * K * LP);
    L.pf = take(8 * (size_t)L.nbt * F * kFSlots);
    L.total = o;
    return L;
}

static void bufs_of(void *ws, const CLayout &L, Bufs *Wp, CBufs *Cp) {
    char *b = static_cast<char *>(ws);
    Bufs W;
    W.g_ent = (float *)(b + L.g_ent); W.g_rel = (float *)(b + L.g_rel); W.g_w = (float *)(b + L.g_w); W.g_b = (float *)(b + L.g_b);
    W.g_vec = nullptr;
    W.s_ent = (grad_t *)(b + L.s_ent); W.s_rel = (grad_t *)(b + L.s_rel); W.s_w = (grad_t *)(b + L.s_w); W.s_b = (grad_t *)(b + L.s_b);
    W.last_h = (int32_t *)(b + L.last_h); W.last_r = (int32_t *)(b + L.last_r); W.last_t = (int32_t *)(b + L.last_t);
    W.last_s = (int32_t *)(b + L.last_s); W.last_n = (int32_t *)(b + L.last_n);
    W.hn = nullptr; W.rn = nullptr; W.out = (float *)(b + L.z2); W.x = (float *)(b + L.x);
    W.dxlab = (float *)(b + L.dxlab); W.dx = (float *)(b + L.dx); W.invh = (float *)(b + L.invh); W.invr = (float *)(b + L.invr);
    W.dtrue = (float *)(b + L.dtrue);
    W.p = (double *)(b + L.p); W.pc = (double *)(b + L.pc); W.sums = (double *)(b + L.sums);
    W.pa = (float *)(b + L.pa); W.pb = (float *)(b + L.pb); W.rowsum = (float *)(b + L.rowsum);
    W.loss_a = (double *)(b + L.loss_a); W.loss_l = (double *)(b + L.loss_l);
    CBufs C;
    C.g_g1 = (float *)(b + L.g_g1); C.g_b1 = (float *)(b + L.g_b1); C.g_kern = (float *)(b + L.g_kern); C.g_cb = (float *)(b + L.g_cb);
    C.g_g2 = (float *)(b + L.g_g2); C.g_b2 = (float *)(b + L.g_b2); C.g_fcw = (float *)(b + L.g_fcw); C.g_fcb = (float *)(b + L.g_fcb);
    C.g_g3 = (float *)(b + L.g_g3); C.g_b3 = (float *)(b + L.g_b3);
    C.img = (float *)(b + L.img); C.s = (float *)(b + L.s); C.dv = (float *)(b + L.dv);
    C.pz = (float *)(b + L.pz); C.dsp = (float *)(b + L.dsp); C.pw = (float *)(b + L.pw); C.pf = (double *)(b + L.pf);
    *Wp = W; *Cp = C;
}

// ---- the dropout mask ----------------------------------------------------------------------------------------------------------
// eight 16-bit lanes of one Philox call: lane l = half l & 1 (0 = low) of word l >> 1
__device__ __forceinline__ uint4 mask_words(const Geo &G, uint32_t layer, uint32_t row, uint32_t group) {
    return oea::philox4x32_10(group, kMaskTag | layer, row, G.step, G.seed_lo, G.seed_hi);
}
__device__ __forceinline__ bool lane_kept(const uint4 &w, int l, uint32_t thr) {
    const uint32_t word = (l >> 1) == 0 ? w.x : (l >> 1) == 1 ? w.y : (l >> 1) == 2 ? w.z : w.w;
    return ((word >> (16 * (l & 1))) & 0xffffu) < thr;
}
__device__ __forceinline__ bool elem_kept(const Geo &G, uint32_t layer, uint32_t row, uint32_t elem) {
    if (G.thr >= 65536u) return true;
    return lane_kept(mask_words(G, layer, row, elem >> 3), (int)(elem & 7u), G.thr);
}

// ---- gather: one wave per batch row ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void conve_gather_kernel(Bufs W, CBufs C, Geo G, const float *__restrict__ ent, const float *__restrict__ rel,
                                                           const float *__restrict__ g1, const float *__restrict__ b1,
                                                           const int32_t *__restrict__ pos, int n_pos, const int32_t *__restrict__ sampled,
                                                           int n_s) {
    const int lane = threadIdx.x & 63;
    const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (int64_t)gridDim.x * 4;
    for (int64_t b = gw; b < n_pos; b += nw) {
        const int32_t h = pos[3 * b], r = pos[3 * b + 1], t = pos[3 * b + 2];
        const float2 a = load2(ent + (int64_t)h * G.ld, G.dim, lane), u = load2(rel + (int64_t)r * G.ld, G.dim, lane);
        const float ia = rsqrtf(fmaxf(dot2(a, a), 1e-12f)), iu = rsqrtf(fmaxf(dot2(u, u), 1e-12f));
        const float v[2][2] = {{a.x * ia, a.y * ia}, {u.x * iu, u.y * iu}};
#pragma unroll
        for (int side = 0; side < 2; ++side)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int c = 2 * lane + e;
                if (c >= G.dim) continue;
                const int p = side * G.dim + c, col = c % G.y;
                const float arg = v[side][e] * (g1[col] * kBnC) + b1[col];
                C.img[b * LP2 + p] = v[side][e];
                C.s[b * LP2 + p] = elem_kept(G, 0u, (uint32_t)b, (uint32_t)p) ? arg * G.inv_keep : 0.f;
            }
        if (lane == 0) {
            W.invh[b] = ia; W.invr[b] = iu;
            W.last_h[b] = h; W.last_r[b] = r; W.last_t[b] = t;
        }
    }
    for (int64_t j = gw * 64 + lane; j < n_s; j += nw * 64) W.last_s[j] = sampled[j];
    if (blockIdx.x == 0 && threadIdx.x == 0) { W.last_n[0] = n_pos; W.last_n[1] = n_s; }
}

// ---- the tile of `a` ----------------------------------------------------------------------------------------------------------------
// 32 rows of s into LDS (stride sp), zero for rows >= n
__device__ __forceinline__ void stage_s(float *Ss, const float *s, const Geo &G, int b0, int n) {
    for (int idx = threadIdx.x; idx < 32 * G.d2; idx += kThreads) {
        const int row = idx / G.d2, p = idx - row * G.d2;
        Ss[row * G.sp + p] = b0 + row < n ? s[(size_t)(b0 + row) * LP2 + p] : 0.f;
    }
}
// 32 rows x LP columns of a batch buffer into an operand tile (stride LDT), zero for rows >= n
__device__ __forceinline__ void stage_z(float *Zs, const float *src, int b0, int n) {
    for (int idx = threadIdx.x; idx < 32 * 32; idx += kThreads) {
        const int row = idx >> 5, c4 = (idx & 31) * 4;
        oea::st4(Zs + row * LDT + c4, b0 + row < n ? oea::ld4(src + (size_t)(b0 + row) * LP + c4) : make_float4(0.f, 0.f, 0.f, 0.f));
    }
}

struct Taps { float w[9]; };
__device__ __forceinline__ Taps load_taps(const float *__restrict__ kern, int F, int f) {
    Taps t;
#pragma unroll
    for (int i = 0; i < 9; ++i) t.w[i] = kern[i * F + f];
    return t;
}
// z1 - cbias at image position (i, j) of the row srow, taps in the order (0,0) (0,1) ... (2,2); v[] receives the nine inputs
__device__ __forceinline__ float conv_at(const float *srow, const Geo &G, const Taps &T, int i, int j, float *v) {
    float z = 0.f;
#pragma unroll
    for (int di = 0; di < 3; ++di)
#pragma unroll
        for (int dj = 0; dj < 3; ++dj) {
            const int ii = i + di - 1, jj = j + dj - 1;
            const float sv = (ii >= 0 && ii < 2 * G.x && jj >= 0 && jj < G.y) ? srow[ii * G.y + jj] : 0.f;
            v[di * 3 + dj] = sv;
            z += sv * T.w[di * 3 + dj];
        }
    return z;
}

// Walks the elements of filter f for 32 rows: item = (row, group of eight elements of the row's K axis).  fn(row, k, z1, u, kept)
template <class Fn>
__device__ __forceinline__ void walk_filter(const float *Ss, const Geo &G, const Taps &T, float cb, float g2c, float b2, int f, int b0, Fn fn) {
    const int e0 = f * G.d2, g_lo = e0 >> 3, ng = ((e0 + G.d2 - 1) >> 3) - g_lo + 1;
    const bool masked = G.thr < 65536u;
    for (int item = threadIdx.x; item < 32 * ng; item += kThreads) {
        const int row = item / ng, g = g_lo + (item - row * ng);
        uint4 w4 = make_uint4(0u, 0u, 0u, 0u);
        if (masked) w4 = mask_words(G, 1u, (uint32_t)(b0 + row), (uint32_t)g);
#pragma unroll
        for (int l = 0; l < 8; ++l) {
            const int k = g * 8 + l - e0;
            if (k < 0 || k >= G.d2) continue;
            const int i = k / G.y, j = k - i * G.y;
            float v[9];
            const float z1 = conv_at(Ss + row * G.sp, G, T, i, j, v) + cb;
            const float u = z1 * g2c + b2;
            const bool kept = !masked || lane_kept(w4, l, G.thr);
            fn(row, k, z1, u, kept, v);
        }
    }
}

__device__ __forceinline__ void build_a_tile(float *As, const float *Ss, const Geo &G, const Taps &T, float cb, float g2c, float b2, int f,
                                             int b0) {
    walk_filter(Ss, G, T, cb, g2c, b2, f, b0, [&](int row, int k, float, float u, bool kept, const float *) {
        As[row * G.ap + k] = (kept && u > 0.f) ? u * G.inv_keep : 0.f;
    });
}

__device__ __forceinline__ int frow(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// ---- forward ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void conve_fwd_kernel(CBufs C, Geo G, const float *__restrict__ kern, const float *__restrict__ cbias,
                                                            const float *__restrict__ g2, const float *__restrict__ b2,
                                                            const float *__restrict__ fcw, int n_pos, int n_split) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *Ss = lds, *As = lds + 32 * G.sp;       // 32 sp is a multiple of 4: As stays 16-byte aligned
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l32 = lane & 31;
    const int b0 = blockIdx.x * 32, split = blockIdx.y;
    const int f0 = (int)((int64_t)split * G.F / n_split), f1 = (int)((int64_t)(split + 1) * G.F / n_split);
    stage_s(Ss, C.s, G, b0, n_pos);
    for (int idx = threadIdx.x; idx < 32 * (G.ap - G.d2); idx += kThreads) {       // the K tail of the tile stays zero
        const int row = idx / (G.ap - G.d2);
        As[row * G.ap + G.d2 + (idx - row * (G.ap - G.d2))] = 0.f;
    }
    const int col = 32 * wave + l32;
    const bool active = 32 * wave < G.dim, col_on = col < G.dim;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int f = f0; f < f1; ++f) {
        __syncthreads();                      // s is staged; the previous filter's reads of As are done
        build_a_tile(As, Ss, G, load_taps(kern, G.F, f), cbias[f], g2[f] * kBnC, b2[f], f, b0);
        __syncthreads();
        if (!active) continue;
        const float *wrow = fcw + (size_t)f * G.d2 * G.ld + col;
        for (int q = 0; q < G.k8; q += 8) {
            const float4 a = oea::ld4(As + l32 * G.ap + q + 4 * half);
            const int k = q + 4 * half;
            float bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) bv[i] = (col_on && k + i < G.d2) ? wrow[(size_t)(k + i) * G.ld] : 0.f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bv[0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bv[1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bv[2], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bv[3], acc, 0, 0, 0);
        }
    }
    const size_t rows_p = (size_t)gridDim.x * 32;
    float *out = C.pz + ((size_t)split * rows_p + b0) * LP;
#pragma unroll
    for (int r = 0; r < 16; ++r) out[(size_t)frow(r, half) * LP + col] = acc[r];
}

// thread = column, block = kRows batch rows: z2 = fcb + the splits in split order, X = relu(z2) gamma3 c + beta3; sum_b X
__global__ __launch_bounds__(LP) void conve_x_kernel(Bufs W, CBufs C, int n_pos, int dim, int rows_p, int n_split,
                                                     const float *__restrict__ fcb, const float *__restrict__ g3,
                                                     const float *__restrict__ b3) {
    const int c = threadIdx.x;
    const int b0 = blockIdx.x * kRows, b1 = min(b0 + kRows, n_pos);
    const bool on = c < dim;
    const float bias = on ? fcb[c] : 0.f, gc = on ? g3[c] * kBnC : 0.f, be = on ? b3[c] : 0.f;
    double s0 = 0;
    for (int b = b0; b < b1; ++b) {
        double zd = (double)bias;
        for (int k = 0; k < n_split; ++k) zd += (double)C.pz[((size_t)k * rows_p + b) * LP + c];
        const float z = on ? (float)zd : 0.f;
        const float x = on ? fmaxf(z, 0.f) * gc + be : 0.f;
        W.out[(size_t)b * LP + c] = z;
        W.x[(size_t)b * LP + c] = x;
        s0 += (double)x;
    }
    W.p[(size_t)blockIdx.x * 4 * LP + c] = s0;
}

// dX = label part + the splits of sweep A + the common vector; dz2 = dX gamma3 c [z2 > 0] over W.dx; sums for gamma3, beta3, fcb
__global__ __launch_bounds__(LP) void conve_dz_kernel(Bufs W, int n_pos, int dim, int rows_p, int n_split, const float *__restrict__ g3) {
    const int c = threadIdx.x;
    const int b0 = blockIdx.x * kRows, b1 = min(b0 + kRows, n_pos);
    const bool on = c < dim;
    const double common = W.sums[16 * LP + c];
    const float gc = on ? g3[c] * kBnC : 0.f;
    double s0 = 0, s1 = 0, s2 = 0;
    for (int b = b0; b < b1; ++b) {
        double gd = (double)W.dxlab[(size_t)b * LP + c] + common;
        for (int k = 0; k < n_split; ++k) gd += (double)W.pa[((size_t)k * rows_p + b) * LP + c];
        const float g = on ? (float)gd : 0.f;
        const float z = W.out[(size_t)b * LP + c];
        const float dz = z > 0.f ? g * gc : 0.f;
        W.dx[(size_t)b * LP + c] = dz;
        s0 += (double)g * (double)(fmaxf(z, 0.f) * kBnC); s1 += (double)g; s2 += (double)dz;
    }
    double *p = W.p + (size_t)blockIdx.x * 4 * LP + c;
    p[0] = s0; p[LP] = s1; p[2 * LP] = s2;
}

// ---- backward-data -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void conve_bwd_data_kernel(Bufs W, CBufs C, Geo G, const float *__restrict__ kern,
                                                                 const float *__restrict__ cbias, const float *__restrict__ g2,
                                                                 const float *__restrict__ b2, const float *__restrict__ fcw, int n_pos,
                                                                 int n_split) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double red[4][kFSums];
    float *Zs = lds, *Da = Zs + 32 * LDT, *Ss = Da + 32 * G.ap, *Ds = Ss + 32 * G.sp;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l32 = lane & 31;
    const int b0 = blockIdx.x * 32, split = blockIdx.y;
    const int f0 = (int)((int64_t)split * G.F / n_split), f1 = (int)((int64_t)(split + 1) * G.F / n_split);
    const int kd8 = (G.dim + 7) & ~7;
    stage_s(Ss, C.s, G, b0, n_pos);
    stage_z(Zs, W.dx, b0, n_pos);
    for (int idx = threadIdx.x; idx < 32 * G.sp; idx += kThreads) Ds[idx] = 0.f;
    for (int f = f0; f < f1; ++f) {
        __syncthreads();                      // the tiles are staged; the previous filter is done with Da
        // da[b][k] = sum_n dz2[b][n] fcW[f 2d + k][n]: wave w takes the k tiles w and w + 4
        for (int ct = wave; 32 * ct < G.d2; ct += 4) {
            const int kk = 32 * ct + l32;
            const bool valid = kk < G.d2;
            const float *wrow = fcw + ((size_t)f * G.d2 + (valid ? kk : 0)) * G.ld;
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            for (int q = 0; q < kd8; q += 8) {
                const int n = q + 4 * half;
                const float4 a = oea::ld4(Zs + l32 * LDT + n);
                const float4 b = (valid && n < G.ld) ? oea::ld4(wrow + n) : make_float4(0.f, 0.f, 0.f, 0.f);   // ld % 4 == 0: inside the row
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
            }
            if (valid)
#pragma unroll
                for (int r = 0; r < 16; ++r) Da[frow(r, half) * G.ap + kk] = acc[r];
        }
        __syncthreads();
        const Taps T = load_taps(kern, G.F, f);
        const float g2c = g2[f] * kBnC;
        float sm[kFSums];
#pragma unroll
        for (int i = 0; i < kFSums; ++i) sm[i] = 0.f;
        walk_filter(Ss, G, T, cbias[f], g2c, b2[f], f, b0, [&](int row, int k, float z1, float u, bool kept, const float *v) {
            const float du = (kept && u > 0.f) ? Da[row * G.ap + k] * G.inv_keep : 0.f;
            const float dz1 = du * g2c;
            sm[0] += du * (z1 * kBnC); sm[1] += du; sm[2] += dz1;
#pragma unroll
            for (int i = 0; i < 9; ++i) sm[3 + i] += dz1 * v[i];
            Da[row * G.ap + k] = dz1;
        });
#pragma unroll
        for (int i = 0; i < kFSums; ++i) {
            const double t = oea::wave_sum_d((double)sm[i]);
            if (lane == 0) red[wave][i] = t;
        }
        __syncthreads();                      // dz1 is in Da, the waves' sums in red
        if (threadIdx.x < kFSums)
            C.pf[((size_t)blockIdx.x * G.F + f) * kFSlots + threadIdx.x] =
                (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
        // the transposed convolution: ds[q] += sum_taps dz1[q - tap] w[tap]; element idx always belongs to the same thread
        for (int idx = threadIdx.x; idx < 32 * G.d2; idx += kThreads) {
            const int row = idx / G.d2, q = idx - row * G.d2, i = q / G.y, j = q - i * G.y;
            float s = 0.f;
#pragma unroll
            for (int di = 0; di < 3; ++di)
#pragma unroll
                for (int dj = 0; dj < 3; ++dj) {
                    const int ii = i - di + 1, jj = j - dj + 1;
                    if (ii >= 0 && ii < 2 * G.x && jj >= 0 && jj < G.y) s += Da[row * G.ap + ii * G.y + jj] * T.w[di * 3 + dj];
                }
            Ds[row * G.sp + q] += s;
        }
    }
    __syncthreads();
    const size_t rows_p = (size_t)gridDim.x * 32;
    for (int idx = threadIdx.x; idx < 32 * G.d2; idx += kThreads) {
        const int row = idx / G.d2, q = idx - row * G.d2;
        C.dsp[((size_t)split * rows_p + b0 + row) * LP2 + q] = Ds[row * G.sp + q];
    }
}

// one wave per batch row: ds = the splits in split order, through drop0 (dv, kept for the column sums), BN1 and the row
// normalisation into the scratch rows of ent[h] and rel[r]
__global__ __launch_bounds__(256) void conve_rows_kernel(Bufs W, CBufs C, Geo G, const float *__restrict__ g1, const int32_t *__restrict__ pos,
                                                         int n_pos, int rows_p, int n_split) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x * 4 + wave;
    if (b >= n_pos) return;
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        float uu[2] = {0.f, 0.f}, gg[2] = {0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int c = 2 * lane + e;
            if (c >= G.dim) continue;
            const int p = side * G.dim + c;
            float ds = 0.f;
            for (int k = 0; k < n_split; ++k) ds += C.dsp[((size_t)k * rows_p + b) * LP2 + p];
            const float dv = elem_kept(G, 0u, (uint32_t)b, (uint32_t)p) ? ds * G.inv_keep : 0.f;
            C.dv[(size_t)b * LP2 + p] = dv;
            uu[e] = C.img[(size_t)b * LP2 + p];
            gg[e] = dv * (g1[c % G.y] * kBnC);
        }
        const float2 u = make_float2(uu[0], uu[1]), g = make_float2(gg[0], gg[1]);
        const float pr = dot2(u, g), inv = side ? W.invr[b] : W.invh[b];
        const int64_t row = pos[3 * b + side];
        grad_t *dst = (side ? W.s_rel : W.s_ent) + row * G.ld;
        const int c = 2 * lane;
        if (c < G.dim) oea::grad_add(dst + c, (g.x - u.x * pr) * inv);
        if (c + 1 < G.dim) oea::grad_add(dst + c + 1, (g.y - u.y * pr) * inv);
    }
}

// thread = image column, block = kRows batch rows: sums for gamma1 and beta1
__global__ __launch_bounds__(LP) void conve_cols_kernel(Bufs W, CBufs C, Geo G, int n_pos) {
    const int j = threadIdx.x;
    const int b0 = blockIdx.x * kRows, b1 = min(b0 + kRows, n_pos);
    double s0 = 0, s1 = 0;
    if (j < G.y)
        for (int b = b0; b < b1; ++b)
            for (int i = 0; i < 2 * G.x; ++i) {
                const size_t at = (size_t)b * LP2 + i * G.y + j;
                const float dv = C.dv[at];
                s0 += (double)dv * (double)(C.img[at] * kBnC); s1 += (double)dv;
            }
    double *p = W.p + (size_t)blockIdx.x * 4 * LP + j;
    p[0] = s0; p[LP] = s1;
}

// ---- backward-weight ---------------------------------------------------------------------------------------------------------------
template <int NT>
__global__ __launch_bounds__(kThreads) void conve_bwd_weight_kernel(Bufs W, CBufs C, Geo G, const float *__restrict__ kern,
                                                                   const float *__restrict__ cbias, const float *__restrict__ g2,
                                                                   const float *__restrict__ b2, int n_pos, int n_split) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *Zs = lds, *As = Zs + 32 * LDT, *Ss = As + 32 * G.ap;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l32 = lane & 31;
    const int f = blockIdx.x, split = blockIdx.y;
    const int n_bt = (n_pos + 31) / 32;
    const int bt0 = (int)((int64_t)split * n_bt / n_split), bt1 = (int)((int64_t)(split + 1) * n_bt / n_split);
    const Taps T = load_taps(kern, G.F, f);
    const float cb = cbias[f], g2c = g2[f] * kBnC, be2 = b2[f];
    f32x16 acc[2][NT];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int y = 0; y < NT; ++y)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][y][r] = 0.f;
    const int km[2] = {32 * wave + l32, 32 * (wave + 4) + l32};
    for (int bt = bt0; bt < bt1; ++bt) {
        const int b0 = bt * 32;
        __syncthreads();                      // the previous tile's reads are done
        stage_s(Ss, C.s, G, b0, n_pos);
        stage_z(Zs, W.dx, b0, n_pos);
        __syncthreads();
        build_a_tile(As, Ss, G, T, cb, g2c, be2, f, b0);
        __syncthreads();
        // dfcW[k][n] += sum_b a[b][k] dz2[b][n]: rows b >= n_pos have dz2 = 0 in Zs
        for (int bb = 0; bb < 32; bb += 2) {
            float av[2], bv[NT];
#pragma unroll
            for (int m = 0; m < 2; ++m) av[m] = km[m] < G.d2 ? As[(bb + half) * G.ap + km[m]] : 0.f;
#pragma unroll
            for (int y = 0; y < NT; ++y) bv[y] = Zs[(bb + half) * LDT + 32 * y + l32];
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int y = 0; y < NT; ++y) acc[m][y] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m], bv[y], acc[m][y], 0, 0, 0);
        }
    }
    float *out = C.pw + ((size_t)split * G.F + f) * G.d2 * LP;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k = 32 * (wave + 4 * m) + frow(r, half);
            if (k < G.d2)
#pragma unroll
                for (int y = 0; y < NT; ++y) out[(size_t)k * LP + 32 * y + l32] = acc[m][y][r];
        }
}

// block = one row of fcW: the splits in split order; the pad columns are zero
__global__ __launch_bounds__(LP) void conve_fcw_kernel(CBufs C, int64_t K, int dim, int ld, int n_split) {
    const int c = threadIdx.x;
    const int64_t k = blockIdx.x;
    if (c >= ld) return;
    float g = 0.f;
    if (c < dim)
        for (int s = 0; s < n_split; ++s) g += C.pw[((size_t)s * K + k) * LP + c];
    C.g_fcw[k * ld + c] = g;
}

// the small gradients out of the fp64 sums: the per-filter partials in row-tile order, the column sums as finalize_kernel left them
__global__ __launch_bounds__(256) void conve_small_kernel(Bufs W, CBufs C, Geo G, int nbt) {
    const double *S1 = W.sums + 4 * LP, *S2 = W.sums + 8 * LP;
    for (int i = threadIdx.x; i < G.F * kFSums; i += 256) {
        const int f = i / kFSums, j = i - f * kFSums;
        double s = 0.0;
        for (int b = 0; b < nbt; ++b) s += C.pf[((size_t)b * G.F + f) * kFSlots + j];
        float *dst = j == 0 ? C.g_g2 + f : j == 1 ? C.g_b2 + f : j == 2 ? C.g_cb + f : C.g_kern + (j - 3) * G.F + f;
        *dst = (float)s;
    }
    for (int c = threadIdx.x; c < LP; c += 256) {
        const bool on = c < G.dim, yon = c < G.y;
        C.g_g3[c] = on ? (float)S1[c] : 0.f;
        C.g_b3[c] = on ? (float)S1[LP + c] : 0.f;
        C.g_fcb[c] = on ? (float)S1[2 * LP + c] : 0.f;
        C.g_g1[c] = yon ? (float)S2[c] : 0.f;
        C.g_b1[c] = yon ? (float)S2[LP + c] : 0.f;
    }
}

static int check_shape(const char *who, int64_t n_ent, int64_t n_rel, int32_t dim, int32_t ld, int32_t F, int64_t max_pos, int64_t max_s) {
    if (!(n_ent > 0 && n_rel > 0 && max_pos >= 0 && max_s >= 0 && n_ent < (1LL << 31) && max_pos < (1LL << 24) && max_s < (1LL << 24))) {
        oea::set_error("%s: invalid argument: table rows / batch capacity", who);
        return OEA_EINVAL;
    }
    if (!(ld % 4 == 0)) { oea::set_error("%s: invalid argument: ld %% 4 == 0", who); return OEA_EINVAL; }
    if (!(dim > 0 && dim <= ld)) { oea::set_error("%s: invalid argument: 0 < dim <= ld", who); return OEA_EINVAL; }
    if (!(F >= 1)) { oea::set_error("%s: invalid argument: filter_num >= 1", who); return OEA_EINVAL; }
    if (dim > kMaxDim) { oea::set_error("%s: dim %d > %d", who, dim, kMaxDim); return OEA_EUNSUPPORTED; }
    if (F > kMaxFilters) { oea::set_error("%s: filter_num %d > %d", who, F, kMaxFilters); return OEA_EUNSUPPORTED; }
    return OEA_OK;
}

template <int NT>
static int launch_weight(dim3 grid, size_t lds, hipStream_t st, const Bufs &W, const CBufs &C, const Geo &G, const float *kern,
                         const float *cbias, const float *g2, const float *b2, int B, int split) {
    OEA_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&conve_bwd_weight_kernel<NT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)lds));
    conve_bwd_weight_kernel<NT><<<grid, kThreads, lds, st>>>(W, C, G, kern, cbias, g2, b2, B, split);
    return OEA_OK;
}

}  // namespace

extern "C" {

size_t oea_conve_workspace_floats(int64_t n_ent, int64_t n_rel, int32_t dim, int32_t ld, int32_t filter_num, int64_t max_pos,
                                  int64_t max_sampled) {
    if (check_shape("oea_conve_workspace_floats", n_ent, n_rel, dim, ld, filter_num, max_pos, max_sampled) != OEA_OK) return 0;
    return make_layout(n_ent, n_rel, dim, ld, filter_num, max_pos, max_sampled).total / 4;
}

int oea_conve_grads(void *workspace, int64_t n_ent, int64_t n_rel, int32_t dim, int32_t ld, int32_t filter_num, int64_t max_pos,
                    int64_t max_sampled, void **grads) {
    const int rc = check_shape("oea_conve_grads", n_ent, n_rel, dim, ld, filter_num, max_pos, max_sampled);
    if (rc != OEA_OK) return rc;
    OEA_REQUIRE(workspace && grads, "null pointer");
    Bufs W;
    CBufs C;
    bufs_of(workspace, make_layout(n_ent, n_rel, dim, ld, filter_num, max_pos, max_sampled), &W, &C);
    float *g[14] = {W.g_ent, W.g_rel, W.g_w, W.g_b, C.g_g1, C.g_b1, C.g_kern, C.g_cb, C.g_g2, C.g_b2, C.g_fcw, C.g_fcb, C.g_g3, C.g_b3};
    for (int i = 0; i < 14; ++i) grads[i] = g[i];
    return OEA_OK;
}

int oea_conve_step(const oea_conve_vars *vars, const oea_conve_cfg *cfg, int64_t n_ent, int64_t n_rel, int32_t dim, int32_t ld,
                   const int32_t *pos, int64_t n_pos, const int32_t *sampled, const float *log_q_sampled, int64_t n_sampled,
                   const int64_t *num_tries, uint64_t mask_step, int64_t t, float lr, void *workspace, int64_t max_pos, int64_t max_sampled,
                   double *loss_accum, int32_t phase, void *stream) {
    OEA_REQUIRE(vars && cfg && workspace && loss_accum, "null pointer");
    for (int i = 0; i < 14; ++i) OEA_REQUIRE(vars->p[i] && vars->m[i] && vars->v[i], "null variable / moment");
    OEA_REQUIRE(phase == OEA_PHASE_BOTH || phase == OEA_PHASE_GRAD || phase == OEA_PHASE_APPLY, "phase");
    const int F = cfg->filter_num;
    const int rc = check_shape("oea_conve_step", n_ent, n_rel, dim, ld, F, max_pos, max_sampled);
    if (rc != OEA_OK) return rc;
    OEA_REQUIRE(cfg->keep_prob > 0.f && cfg->keep_prob <= 1.f, "0 < keep_prob <= 1");
    OEA_REQUIRE(n_pos >= 1 && n_pos <= max_pos && pos, "1 <= n_pos <= max_pos");
    OEA_REQUIRE(n_sampled >= 2 && n_sampled <= max_sampled && n_sampled <= n_ent, "2 <= n_sampled <= min(max_sampled, n_ent)");
    OEA_REQUIRE(sampled && log_q_sampled && num_tries, "sampled / log_q_sampled / num_tries");
    OEA_REQUIRE(t >= 1, "t >= 1");
    hipStream_t st = oea::as_stream(stream);
    const CLayout L = make_layout(n_ent, n_rel, dim, ld, F, max_pos, max_sampled);
    Bufs W;
    CBufs C;
    bufs_of(workspace, L, &W, &C);
    const int B = (int)n_pos, S = (int)n_sampled;
    const int nbt = (B + 31) / 32, nct = (S + 31) / 32, nwb = (B + 3) / 4;
    const int64_t K = (int64_t)2 * dim * F;
    float *const *p = vars->p;
    const float *ent = p[0], *rel = p[1], *ent_w = p[2], *ent_b = p[3], *g1 = p[4], *b1 = p[5], *kern = p[6], *cbias = p[7], *g2 = p[8],
                *b2 = p[9], *fcw = p[10], *fcb = p[11], *g3 = p[12], *b3 = p[13];
    if (phase != OEA_PHASE_APPLY) {
        Geo G;
        G.dim = dim; G.ld = ld; G.F = F; G.d2 = 2 * dim;
        factorize(dim, &G.x, &G.y);
        G.k8 = (G.d2 + 7) & ~7; G.ap = G.k8 + 4;
        G.sp = G.d2 + 1;                      // odd: the rows of a tile start on different banks
        G.inv_keep = 1.f / cfg->keep_prob;
        G.thr = cfg->keep_prob >= 1.f ? 65536u : (uint32_t)floor((double)cfg->keep_prob * 65536.0);
        G.seed_lo = (uint32_t)cfg->seed; G.seed_hi = (uint32_t)(cfg->seed >> 32); G.step = (uint32_t)mask_step;
        const int split_a = split_of(nbt, nct), split_b = split_of(nct, nbt);
        const int split_f = split_of(nbt, F), split_w = split_of(F, nbt);
        const int nt = (dim + 31) / 32;
        const int64_t cap = std::max(max_pos, max_sampled);
        const size_t lds_f = 4 * (size_t)32 * (G.sp + G.ap), lds_d = 4 * (size_t)32 * (LDT + G.ap + 2 * G.sp),
                     lds_w = 4 * (size_t)32 * (LDT + G.ap + G.sp);
        OEA_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&conve_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)lds_f));
        OEA_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&conve_bwd_data_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)lds_d));
        clear_prev_kernel<<<(unsigned)std::min<int64_t>(oea::ceil_div(cap, 4), 4096), 256, 0, st>>>(W, ld, cap);
        conve_gather_kernel<<<(unsigned)std::min<int64_t>(oea::ceil_div(std::max(B, (S + 63) / 64), 4), 4096), 256, 0, st>>>(
            W, C, G, ent, rel, g1, b1, pos, B, sampled, S);
        conve_fwd_kernel<<<dim3(nbt, split_f), kThreads, lds_f, st>>>(C, G, kern, cbias, g2, b2, fcw, B, split_f);
        conve_x_kernel<<<nbt, LP, 0, st>>>(W, C, B, dim, nbt * 32, split_f, fcb, g3, b3);
        finalize_kernel<<<1, LP * kChains, 0, st>>>(W.p, nbt, 1, W.sums);
        label_kernel<false><<<nwb, 256, 0, st>>>(W, B, dim, ld, nullptr, ent_w, ent_b, pos, num_tries, 1.0 / log((double)n_ent + 1.0));
        SweepArgs A;
        A.bias = ent_b; A.logq = log_q_sampled; A.cand_ids = sampled; A.dim = dim;
        A.f_src = W.x; A.f_ids = nullptr; A.f_ld = LP; A.n_f = B;
        A.g_src = ent_w; A.g_ids = sampled; A.g_ld = ld; A.n_g = S;
        A.n_split = split_a; A.partial = W.pa; A.rowsum = nullptr; A.loss = W.loss_a;
        launch_sweep<false>(nt, dim3(nbt, split_a), st, A);
        cand_const_kernel<<<nct, LP, 0, st>>>(W, ent_w, ent_b, sampled, log_q_sampled, S, dim, ld);
        finalize_kernel<<<1, LP * kChains, 0, st>>>(W.pc, nct, 1, W.sums + 16 * LP);
        SweepArgs Bq = A;
        Bq.f_src = ent_w; Bq.f_ids = sampled; Bq.f_ld = ld; Bq.n_f = S;
        Bq.g_src = W.x; Bq.g_ids = nullptr; Bq.g_ld = LP; Bq.n_g = B;
        Bq.n_split = split_b; Bq.partial = W.pb; Bq.rowsum = W.rowsum; Bq.loss = nullptr;
        launch_sweep<true>(nt, dim3(nct, split_b), st, Bq);
        reduce_cand_kernel<false><<<S, LP, 0, st>>>(W, sampled, log_q_sampled, ent_b, nullptr, W.sums, B, S, nct * 32, split_b, dim, ld);
        conve_dz_kernel<<<nbt, LP, 0, st>>>(W, B, dim, nbt * 32, split_a, g3);
        finalize_kernel<<<1, LP * kChains, 0, st>>>(W.p, nbt, 3, W.sums + 4 * LP);
        conve_bwd_data_kernel<<<dim3(nbt, split_f), kThreads, lds_d, st>>>(W, C, G, kern, cbias, g2, b2, fcw, B, split_f);
        conve_rows_kernel<<<nwb, 256, 0, st>>>(W, C, G, g1, pos, B, nbt * 32, split_f);
        conve_cols_kernel<<<nbt, LP, 0, st>>>(W, C, G, B);
        finalize_kernel<<<1, LP * kChains, 0, st>>>(W.p, nbt, 2, W.sums + 8 * LP);
        int r;
        const dim3 gw(F, split_w);
        switch (nt) {
            case 1: r = launch_weight<1>(gw, lds_w, st, W, C, G, kern, cbias, g2, b2, B, split_w); break;
            case 2: r = launch_weight<2>(gw, lds_w, st, W, C, G, kern, cbias, g2, b2, B, split_w); break;
            case 3: r = launch_weight<3>(gw, lds_w, st, W, C, G, kern, cbias, g2, b2, B, split_w); break;
            default: r = launch_weight<4>(gw, lds_w, st, W, C, G, kern, cbias, g2, b2, B, split_w); break;
        }
        if (r != OEA_OK) return r;
        conve_fcw_kernel<<<(unsigned)K, LP, 0, st>>>(C, K, dim, ld, split_w);
        conve_small_kernel<<<1, 256, 0, st>>>(W, C, G, nbt);
        convert_kernel<<<(unsigned)std::min<int64_t>(oea::ceil_div(std::max(B, S), 4), 4096), 256, 0, st>>>(W, ld, B, S);
        loss_kernel<<<1, 64, 0, st>>>(W.loss_l, nwb, W.loss_a, nbt * split_a, loss_accum);
        OEA_CHECK_HIP(hipGetLastError());
    }
    if (phase != OEA_PHASE_GRAD) {
        int x, y;
        factorize(dim, &x, &y);
        const float *g[14] = {W.g_ent, W.g_rel, W.g_w, W.g_b, C.g_g1, C.g_b1, C.g_kern, C.g_cb, C.g_g2, C.g_b2, C.g_fcw, C.g_fcb, C.g_g3, C.g_b3};
        const int64_t n[14] = {n_ent * ld, n_rel * ld, n_ent * ld, n_ent, y, y, 9 * F, F, F, F, K * ld, dim, dim, dim};
        for (int i = 0; i < 14; ++i) {
            const int r = oea_adam_dense(vars->p[i], g[i], vars->m[i], vars->v[i], n[i], lr, 0.9f, 0.999f, 1e-8f, t, stream);
            if (r != OEA_OK) return r;
        }
    }
    return OEA_OK;
}

}  // extern "C"
