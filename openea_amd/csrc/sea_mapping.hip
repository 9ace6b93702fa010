// sea_mapping.hip -- SEA's two-way, cycle-consistent mapping step, fused.
//
// Replaces session.run([mapping_loss, mapping_optimizer]) of approaches/sea.py:73-98,129-145:
//     E = l2_normalize(ent, 1);  L1 = E[a], L2 = E[b] (labelled links), U1 = E[c], U2 = E[d] (unlabelled links)
//     Y12 = gl2n(L1 M1)   Y21 = gl2n(L2 M2)   Y121 = gl2n(U1 M1 M2)   Y212 = gl2n(U2 M2 M1)
//     loss = alpha_1 (|L2 - Y12|^2 + |L1 - Y21|^2) + alpha_2 (|U1 - Y121|^2 + |U2 - Y212|^2)
// gl2n is tf.nn.l2_normalize WITHOUT an axis: the whole [n, d] block divided by s = sqrt(max(sum of all its squares, 1e-12)).
// For Y = P / s with upstream G:  dP = (G - Y <G, Y>_F) / s  -- block-wide scalars, which force kernel boundaries:
//
//   F1  one wave per link end: gather + row-normalise, x M_h with M_h in LDS (h = 0: L1, U1 on M1; h = 1: L2, U2 on M2):
//       P12 / P21 and A1 = U1 M1 / A2 = U2 M2, the row's sum of squares
//   F2  Q121 = A1 M2, Q212 = A2 M1, the row's sum of squares
//   R   block sums of squares (every workgroup adds the same row values in the same order), residual e = T - Y per row,
//       the row's share of the loss and of <e, Y>
//   B1  block inner products the same way; dP / dQ per row, the direct term 2 alpha e into the target's entity row, dP M_h^T:
//       labelled -> entity row, unlabelled -> dA
//   B2  dA M_h^T -> entity row
//   G   dM_h = XA_h^T GB_h with XA_1 = [L1; U1; A2], GB_1 = [dP12; dA1; dQ212] (XA_2 = [L2; U2; A1], GB_2 = [dP21; dA2; dQ121]):
//       the row-chunked fp32 matrix-core product of gemm_tn.hip into per-chunk partials
//   U   chunks added in chunk order, SGD / Adam on M1 and M2 in place; the loss from the row shares in a fixed order
//
// No float atomics on anything M1 / M2 depend on: the same bits run to run.  The entity-row gradients go into the step
// engine's scratch (oea::grad_add) and oea_triple_step_phase(..., OEA_PHASE_APPLY) finishes the step, as for oea_mapping_step.
#include "common.h"

#include <algorithm>
#include <cmath>

extern "C" int oea_gemm_tn_plan(int64_t m, int32_t k1, int32_t k2, int32_t *chunks, int64_t *rows_per_chunk);
extern "C" int oea_gemm_tn_partial(const float *a, int32_t lda, int32_t k1, const float *b, int32_t ldb, int32_t k2, int64_t m,
                                   int32_t chunk_begin, int32_t chunk_end, float *workspace, void *stream);

namespace {

constexpr int kMaxDim = 128;

struct SeaArgs {
    const float *ent;
    int ld, dim, d4, l2norm;
    const int32_t *ids[2][2];        // [h][0]: labelled ids of side h (l1 / l2), [h][1]: unlabelled (u1 / u2)
    int n_l, n_u;
    const float *M[2];
    float alpha[2];                  // labelled, unlabelled
    float *xa[2], *gb[2], *p[2];     // [rows, ld]; xa / gb: n_l + 2 n_u rows, p: n_l + n_u rows
    float *sq[2], *rl[2], *rd[2];    // per row of p[h]: sum of squares, loss share, <e, Y> share
    float *un[2];                    // per gathered row of xa[h]: 1 when the row was normalised to unit length (not clamped)
    oea::grad_t *eg;
    oea::flag_t *et;
};

enum { PH_F1 = 0, PH_F2 = 1, PH_B1 = 2, PH_B2 = 3 };

// sum of arr[0, n) as the same double in every thread of every workgroup: thread t adds t, t + 256, ... then a fixed tree
__device__ double block_sum(const float *__restrict__ arr, int n, double *red) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += (double)arr[i];
    __syncthreads();
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    return red[0];
}

// the block's scale: s = sqrt(max(ss, 1e-12)); unit = the block was not clamped (then |Y|_F = 1 and dP carries the <G, Y> term)
struct BlockNorm { float inv; bool unit; };
__device__ __forceinline__ BlockNorm block_norm(double ss) {
    BlockNorm b;
    b.unit = ss >= 1e-12;
    b.inv = (float)(1.0 / sqrt(b.unit ? ss : 1e-12));
    return b;
}

// y[c] = sum_k x[k] Ms[k * dim + c] for c = lane, lane + 64 (x: d4 floats in LDS, zero past dim; Ms: d4 x dim, rows past dim zero)
__device__ __forceinline__ void row_times(const float *x, const float *Ms, int dim, int d4, int lane, float &y0, float &y1) {
    const int c0 = lane < dim ? lane : 0, c1 = lane + 64 < dim ? lane + 64 : 0;
    const float *m0 = Ms + c0, *m1 = Ms + c1;
    float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;
    for (int k = 0; k < d4; k += 4) {
        const float4 xv = *reinterpret_cast<const float4 *>(x + k);
        a0 = fmaf(xv.x, m0[(k + 0) * dim], a0);
        a1 = fmaf(xv.x, m1[(k + 0) * dim], a1);
        b0 = fmaf(xv.y, m0[(k + 1) * dim], b0);
        b1 = fmaf(xv.y, m1[(k + 1) * dim], b1);
        a0 = fmaf(xv.z, m0[(k + 2) * dim], a0);
        a1 = fmaf(xv.z, m1[(k + 2) * dim], a1);
        b0 = fmaf(xv.w, m0[(k + 3) * dim], b0);
        b1 = fmaf(xv.w, m1[(k + 3) * dim], b1);
    }
    y0 = a0 + b0;
    y1 = a1 + b1;
}

// the target T of row r of p[s] and the entity it came from: labelled rows face the other side's labelled rows, unlabelled rows
// their own side's
__device__ __forceinline__ const float *target_row(const SeaArgs &a, int s, int r, int *ent_id) {
    const bool lab = r < a.n_l;
    const int side = lab ? 1 - s : s;
    *ent_id = lab ? a.ids[side][0][r] : a.ids[side][1][r - a.n_l];
    return a.xa[side] + (int64_t)r * a.ld;
}

// Grid: blocks [0, gridDim.x / 2) are half h = 0, the rest h = 1; every workgroup stages ONE matrix (transposed for the backward
// phases) and its four waves walk the half's rows.
template <int PH>
__global__ __launch_bounds__(256) void sea_rows_kernel(const SeaArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];          // Ms [d4 x dim], then per wave x [d4]
    __shared__ double red[256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nbh = gridDim.x >> 1;
    const int h = (int)blockIdx.x >= nbh ? 1 : 0, bh = (int)blockIdx.x - h * nbh;
    const int dim = a.dim, d4 = a.d4, ld = a.ld, n_l = a.n_l, n_u = a.n_u;
    float *Ms = lds, *x = lds + d4 * dim + wave * d4;
    // F1: M_h;  F2: in = A of the other side, matrix of the other side;  B1 / B2: M_h^T
    const float *Mg = a.M[PH == PH_F2 ? 1 - h : h];
    for (int i = threadIdx.x; i < d4 * dim; i += 256) {
        const int k = i / dim, c = i - k * dim;
        Ms[i] = k < dim ? ((PH == PH_B1 || PH == PH_B2) ? Mg[c * dim + k] : Mg[i]) : 0.f;
    }
    // B1: the scalars of the two blocks this half differentiates: its own side's labelled block and the other side's unlabelled
    BlockNorm nrm[2] = {{0.f, false}, {0.f, false}};
    float cdot[2] = {0.f, 0.f};
    if (PH == PH_B1) {
        nrm[0] = block_norm(block_sum(a.sq[h], n_l, red));
        nrm[1] = block_norm(block_sum(a.sq[1 - h] + n_l, n_u, red));
        cdot[0] = nrm[0].unit ? (float)block_sum(a.rd[h], n_l, red) : 0.f;
        cdot[1] = nrm[1].unit ? (float)block_sum(a.rd[1 - h] + n_l, n_u, red) : 0.f;
    }
    __syncthreads();
    const int rows = (PH == PH_F1 || PH == PH_B1) ? n_l + n_u : n_u;
    const int c0 = lane, c1 = lane + 64;
    for (int r = bh * 4 + wave; r < rows; r += nbh * 4) {
        int out_ent = -1;               // entity row that takes y = x Ms (backward phases)
        if (PH == PH_F1) {
            const bool lab = r < n_l;
            const int id = lab ? a.ids[h][0][r] : a.ids[h][1][r - n_l];
            const float *row = a.ent + (int64_t)id * ld;
            const float u0 = c0 < dim ? row[c0] : 0.f, u1 = c1 < dim ? row[c1] : 0.f;
            const float ss = oea::group_sum<64>(u0 * u0 + u1 * u1);
            const float inv = a.l2norm ? rsqrtf(fmaxf(ss, 1e-12f)) : 1.f;
            float *xo = a.xa[h] + (int64_t)r * ld;
            if (c0 < ld) xo[c0] = u0 * inv;
            if (c1 < ld) xo[c1] = u1 * inv;
            for (int c = c1 + 64; c < ld; c += 64) xo[c] = 0.f;
            if (c0 < d4) x[c0] = u0 * inv;
            if (c1 < d4) x[c1] = u1 * inv;
            if (lane == 0) { a.et[id] = 1.f; a.un[h][r] = (a.l2norm && ss >= 1e-12f) ? 1.f : 0.f; }
        } else if (PH == PH_F2) {
            const float *in = a.xa[1 - h] + (int64_t)(n_l + n_u + r) * ld;
            if (c0 < d4) x[c0] = in[c0];
            if (c1 < d4) x[c1] = in[c1];
        } else if (PH == PH_B2) {
            const float *in = a.gb[h] + (int64_t)(n_l + r) * ld;
            if (c0 < d4) x[c0] = in[c0];
            if (c1 < d4) x[c1] = in[c1];
            out_ent = a.ids[h][1][r];
        } else {                        // B1: dP of row r of its source block
            const bool lab = r < n_l;
            const int s = lab ? h : 1 - h, b = lab ? 0 : 1;
            int t_ent;
            const float *T = target_row(a, s, r, &t_ent);
            const float *P = a.p[s] + (int64_t)r * ld;
            const float al = a.alpha[b], inv = nrm[b].inv;
            float *gout = a.gb[h] + (int64_t)(lab ? r : r + n_u) * ld;
            // The direct term d loss / d T = 2 alpha (T - Y).  When T is a row-normalised table row, the normalisation's
            // Jacobian (I - T T^T) / |raw| annihilates the 2 alpha T part exactly, and the optimiser pass would take it out again
            // by subtracting two numbers a hundred times the size of what is left: only -2 alpha Y goes into the scratch then.
            // (A row under the 1e-12 clamp is shorter than one and keeps the whole term.)
            const float t0 = c0 < dim ? T[c0] : 0.f, t1 = c1 < dim ? T[c1] : 0.f;
            const bool t_unit = a.un[lab ? 1 - s : s][r] != 0.f;
            float dp[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int c = lane + 64 * j;
                dp[j] = 0.f;
                if (c < dim) {
                    const float tc = j ? t1 : t0, y = P[c] * inv, e = tc - y;
                    dp[j] = -2.f * al * (e - y * cdot[b]) * inv;
                    oea::grad_add(a.eg + (int64_t)t_ent * ld + c, 2.f * al * (t_unit ? -y : e));
                }
                if (c < ld) gout[c] = dp[j];
                if (c < d4) x[c] = dp[j];
            }
            for (int c = c1 + 64; c < ld; c += 64) gout[c] = 0.f;
            out_ent = lab ? a.ids[h][0][r] : -1;
        }
        __builtin_amdgcn_wave_barrier();
        float y0, y1;
        row_times(x, Ms, dim, d4, lane, y0, y1);
        if (c0 >= dim) y0 = 0.f;
        if (c1 >= dim) y1 = 0.f;
        if (PH == PH_F1 || PH == PH_F2) {
            const bool lab = PH == PH_F1 && r < n_l;
            // F1 labelled: P_h[r];  F1 unlabelled: A -> the other side's xa tail;  F2: Q -> P_h[n_l + r]
            float *out = PH == PH_F2 ? a.p[h] + (int64_t)(n_l + r) * ld
                                     : (lab ? a.p[h] + (int64_t)r * ld : a.xa[1 - h] + (int64_t)(r + n_u) * ld);
            if (c0 < ld) out[c0] = y0;
            if (c1 < ld) out[c1] = y1;
            for (int c = c1 + 64; c < ld; c += 64) out[c] = 0.f;
            if (PH == PH_F2 || lab) {
                const float ss = oea::group_sum<64>(y0 * y0 + y1 * y1);
                if (lane == 0) a.sq[h][PH == PH_F2 ? n_l + r : r] = ss;
            }
        } else if (out_ent >= 0) {
            if (c0 < dim) oea::grad_add(a.eg + (int64_t)out_ent * ld + c0, y0);
            if (c1 < dim) oea::grad_add(a.eg + (int64_t)out_ent * ld + c1, y1);
        } else {                        // B1 unlabelled: dA of the other side, for B2 and for dM
            float *out = a.gb[1 - h] + (int64_t)r * ld;
            if (c0 < ld) out[c0] = y0;
            if (c1 < ld) out[c1] = y1;
            for (int c = c1 + 64; c < ld; c += 64) out[c] = 0.f;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// R: residuals.  One wave per row of p[0] and p[1]; rl = sum e^2, rd = sum e Y with Y = P / s, e = T - Y.
__global__ __launch_bounds__(256) void sea_resid_kernel(const SeaArgs a) {
    __shared__ double red[256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n_l = a.n_l, n_u = a.n_u, n = n_l + n_u, dim = a.dim;
    float inv[2][2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        inv[s][0] = block_norm(block_sum(a.sq[s], n_l, red)).inv;
        inv[s][1] = block_norm(block_sum(a.sq[s] + n_l, n_u, red)).inv;
    }
    for (int i = blockIdx.x * 4 + wave; i < 2 * n; i += gridDim.x * 4) {
        const int s = i >= n ? 1 : 0, r = i - s * n;
        int t_ent;
        const float *T = target_row(a, s, r, &t_ent);
        const float *P = a.p[s] + (int64_t)r * a.ld;
        const float iv = inv[s][r < n_l ? 0 : 1];
        float l = 0.f, d = 0.f;
        for (int c = lane; c < dim; c += 64) {
            const float y = P[c] * iv, e = T[c] - y;
            l = fmaf(e, e, l);
            d = fmaf(e, y, d);
        }
        l = oea::group_sum<64>(l);
        d = oea::group_sum<64>(d);
        if (lane == 0) { a.rl[s][r] = l; a.rd[s][r] = d; }
    }
}

// U: dM_h = its chunks in chunk order; SGD / Adam (training_ops ApplyAdam, as apply_rows_dense) on M_h in place.  blockIdx.y = h.
// Workgroup (0, 0) also adds the step's loss from the row shares.
__global__ __launch_bounds__(256) void sea_update_kernel(const SeaArgs a, float *M1, float *M2, float *state,
                                                         const float *__restrict__ partials, int chunks, int opt_kind, float lr,
                                                         float lr_t, float beta1, float beta2, float eps,
                                                         double *__restrict__ loss_accum) {
    __shared__ double red[256];
    const int h = blockIdx.y, dim = a.dim, ld = a.ld;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < dim * dim) {
        const int k = idx / dim, c = idx - k * dim;
        const int64_t stride = (int64_t)ld * ld;
        const float *p = partials + (int64_t)h * chunks * stride + (int64_t)k * ld + c;
        float g = 0.f;
#pragma unroll 4
        for (int q = 0; q < chunks; ++q) g += p[q * stride];
        float *M = h ? M2 : M1;
        if (opt_kind == OEA_OPT_ADAM) {
            float *mp = state + (int64_t)(2 * h) * dim * dim + idx, *vp = mp + (int64_t)dim * dim;
            const float m = *mp + (g - *mp) * (1.f - beta1);
            const float v = *vp + (g * g - *vp) * (1.f - beta2);
            *mp = m;
            *vp = v;
            M[idx] = M[idx] - lr_t * m / (sqrtf(v) + eps);
        } else {
            M[idx] = M[idx] - lr * g;
        }
    }
    if (blockIdx.x == 0 && blockIdx.y == 0) {
        const int n_l = a.n_l, n_u = a.n_u;
        const double lab = block_sum(a.rl[0], n_l, red) + block_sum(a.rl[1], n_l, red);
        const double unl = block_sum(a.rl[0] + n_l, n_u, red) + block_sum(a.rl[1] + n_l, n_u, red);
        if (threadIdx.x == 0) atomicAdd(loss_accum, (double)a.alpha[0] * lab + (double)a.alpha[1] * unl);
    }
}

int64_t round4(int64_t v) { return (v + 3) / 4 * 4; }

int gemm_chunks(int64_t m, int ld) {
    int32_t chunks = 1;
    int64_t rpc = 0;
    if (m > 0) (void)oea_gemm_tn_plan(m, ld, ld, &chunks, &rpc);
    return chunks;
}

template <int PH>
int launch_rows(const SeaArgs &a, int rows, hipStream_t st) {
    if (rows <= 0) return OEA_OK;
    const size_t lds = sizeof(float) * ((size_t)a.d4 * a.dim + 4 * (size_t)a.d4);
    // the attribute belongs to (function, device): set on every call
    OEA_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&sea_rows_kernel<PH>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)(sizeof(float) * ((size_t)kMaxDim * kMaxDim + 4 * kMaxDim))));
    const unsigned nbh = (unsigned)std::min<int64_t>(std::max<int64_t>(oea::ceil_div(rows, 16), 1), 256);
    sea_rows_kernel<PH><<<2 * nbh, 256, lds, st>>>(a);
    return OEA_OK;
}

int check_args(int32_t ld, int32_t dim, int64_t n_l, int64_t n_u, const oea_step_cfg *cfg, const float *M_state) {
    OEA_REQUIRE(cfg, "null pointer");
    OEA_REQUIRE(dim > 0 && dim <= ld && ld % 4 == 0, "ld % 4 == 0 and dim <= ld");
    OEA_REQUIRE(n_l >= 0 && n_u >= 0 && n_l + n_u > 0 && n_l + 2 * n_u < (1 << 28), "0 < n_l + n_u");
    if (dim > kMaxDim || (cfg->opt_kind != OEA_OPT_SGD && cfg->opt_kind != OEA_OPT_ADAM)) {
        oea::set_error("oea_sea_mapping_step: dim <= 128 and SGD or Adam (got dim %d, opt_kind %d)", dim, cfg->opt_kind);
        return OEA_EUNSUPPORTED;
    }
    if (cfg->opt_kind == OEA_OPT_ADAM) {
        OEA_REQUIRE(M_state, "Adam needs the moments of M1 and M2");
        OEA_REQUIRE(cfg->opt_t >= 1 && cfg->beta1 > 0.f && cfg->beta1 < 1.f && cfg->eps > 0.f, "Adam: opt_t = 1-based step count; beta1 / eps");
    }
    return OEA_OK;
}

}  // namespace

extern "C" {

size_t oea_sea_mapping_workspace_floats(int64_t n_l, int64_t n_u, int32_t ld, int32_t dim) {
    (void)dim;
    if (n_l < 0 || n_u < 0 || ld <= 0) return 0;
    const int64_t m = n_l + 2 * n_u, n = n_l + n_u;
    return (size_t)(4 * m * ld + 2 * n * ld + 8 * round4(n) + 2 * (int64_t)gemm_chunks(m, ld) * ld * ld + 64);
}

int oea_sea_mapping_step(const float *ent, int32_t ld, int32_t dim, const int32_t *ids_l1, const int32_t *ids_l2, int64_t n_l,
                         const int32_t *ids_u1, const int32_t *ids_u2, int64_t n_u, float *M1, float *M2, float *M_state,
                         float alpha_1, float alpha_2, const oea_step_cfg *cfg, void *ent_grad, void *ent_touched, float *work,
                         double *loss_accum, void *stream) {
    int rc = check_args(ld, dim, n_l, n_u, cfg, M_state);
    if (rc != OEA_OK) return rc;
    OEA_REQUIRE(ent && M1 && M2 && ent_grad && ent_touched && work && loss_accum, "null pointer");
    OEA_REQUIRE((ids_l1 && ids_l2) || n_l == 0, "labelled ids");
    OEA_REQUIRE((ids_u1 && ids_u2) || n_u == 0, "unlabelled ids");
    OEA_REQUIRE(((uintptr_t)work & 15) == 0, "16-byte aligned workspace");
    hipStream_t st = oea::as_stream(stream);
    const int64_t m = n_l + 2 * n_u, n = n_l + n_u;
    SeaArgs a;
    a.ent = ent; a.ld = ld; a.dim = dim; a.d4 = (int)round4(dim); a.l2norm = cfg->ent_l2_norm;
    a.ids[0][0] = ids_l1; a.ids[1][0] = ids_l2; a.ids[0][1] = ids_u1; a.ids[1][1] = ids_u2;
    a.n_l = (int)n_l; a.n_u = (int)n_u;
    a.M[0] = M1; a.M[1] = M2;
    a.alpha[0] = alpha_1; a.alpha[1] = alpha_2;
    float *w = work;
    for (int h = 0; h < 2; ++h) { a.xa[h] = w; w += m * ld; }
    for (int h = 0; h < 2; ++h) { a.gb[h] = w; w += m * ld; }
    for (int h = 0; h < 2; ++h) { a.p[h] = w; w += n * ld; }
    for (int h = 0; h < 2; ++h) { a.sq[h] = w; w += round4(n); a.rl[h] = w; w += round4(n); a.rd[h] = w; w += round4(n); a.un[h] = w; w += round4(n); }
    float *partials = w;
    a.eg = static_cast<oea::grad_t *>(ent_grad);
    a.et = static_cast<oea::flag_t *>(ent_touched);
    const int chunks = gemm_chunks(m, ld);

    if ((rc = launch_rows<PH_F1>(a, (int)n, st)) != OEA_OK) return rc;
    if ((rc = launch_rows<PH_F2>(a, (int)n_u, st)) != OEA_OK) return rc;
    sea_resid_kernel<<<(unsigned)std::min<int64_t>(oea::ceil_div(2 * n, 8), 512), 256, 0, st>>>(a);
    if ((rc = launch_rows<PH_B1>(a, (int)n, st)) != OEA_OK) return rc;
    if ((rc = launch_rows<PH_B2>(a, (int)n_u, st)) != OEA_OK) return rc;
    for (int h = 0; h < 2; ++h) {
        rc = oea_gemm_tn_partial(a.xa[h], ld, ld, a.gb[h], ld, ld, m, 0, chunks, partials + (int64_t)h * chunks * ld * ld, stream);
        if (rc != OEA_OK) return rc;
    }
    const double t = (double)cfg->opt_t;
    const float lr_t = cfg->opt_kind == OEA_OPT_ADAM
                           ? (float)((double)cfg->lr * std::sqrt(1.0 - std::pow((double)cfg->beta2, t)) / (1.0 - std::pow((double)cfg->beta1, t)))
                           : cfg->lr;
    sea_update_kernel<<<dim3((unsigned)oea::ceil_div((int64_t)dim * dim, 256), 2), 256, 0, st>>>(
        a, M1, M2, M_state, partials, chunks, cfg->opt_kind, cfg->lr, lr_t, cfg->beta1, cfg->beta2, cfg->eps, loss_accum);
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

// A whole mapping epoch of SEA (approaches/sea.py:129-145) enqueued by ONE call: per step the fused mapping step above + the
// apply phase of the step engine with `cfg` (the mapping optimiser's own Adam state and step count).  batches: device int32
// [steps][l1 (n_l) | l2 (n_l) | u1 (n_u) | u2 (n_u)].
int oea_sea_mapping_epoch(float *ent, float *ent_acc, int64_t n_ent, float *rel, float *rel_acc, int64_t n_rel, int32_t dim,
                          int32_t ld, const int32_t *batches, int32_t steps, int64_t n_l, int64_t n_u, float *M1, float *M2,
                          float *M_state, float alpha_1, float alpha_2, const oea_step_cfg *cfg, void *workspace, float *work,
                          double *mapping_loss_accum, double *step_loss_accum, void *stream) {
    int rc = check_args(ld, dim, n_l, n_u, cfg, M_state);
    if (rc != OEA_OK) return rc;
    OEA_REQUIRE(ent && rel && batches && M1 && M2 && workspace && work && mapping_loss_accum && step_loss_accum, "null pointer");
    OEA_REQUIRE(steps >= 0, "steps >= 0");
    void *eg = nullptr, *et = nullptr;
    rc = oea_step_entity_scratch(workspace, n_ent, n_rel, ld, &eg, &et);
    if (rc != OEA_OK) return rc;
    oea_step_cfg step_cfg = *cfg;
    for (int32_t s = 0; s < steps; ++s) {
        const int32_t *l1 = batches + (int64_t)s * 2 * (n_l + n_u), *l2 = l1 + n_l, *u1 = l2 + n_l, *u2 = u1 + n_u;
        rc = oea_sea_mapping_step(ent, ld, dim, l1, l2, n_l, u1, u2, n_u, M1, M2, M_state, alpha_1, alpha_2, &step_cfg, eg, et, work,
                                  mapping_loss_accum, stream);
        if (rc != OEA_OK) return rc;
        rc = oea_triple_step_phase(ent, ent_acc, n_ent, rel, rel_acc, n_rel, dim, ld, nullptr, 0, nullptr, 0, &step_cfg, workspace,
                                   step_loss_accum, OEA_PHASE_APPLY, stream);
        if (rc != OEA_OK) return rc;
        ++step_cfg.opt_t;
    }
    return OEA_OK;
}

}  // extern "C"
