// semantic_step.hip -- the training step of the semantic-matching models HolE (models/semantic/hole.py:41-86 of the
// reference), SimplE (models/semantic/simple.py:39-88) and DistMult (models/semantic/distmult.py:43-59).
//
//   HolE    u = l2n(ent)[e], rh = l2n(l2n(rel)[r]) (the relation row is normalised twice, hole.py:57),
//           c[k] = sum_i uh[i] ut[(i + k) mod d] (circular correlation), score = -sigmoid(rh . c),
//           loss = sum_p relu(margin + score_p - mean_j score_{p,j}) over the k negatives neg[p k .. p k + k).
//   SimplE  four tables stacked in two: ent rows [0, E) = H, [E, 2E) = T; rel rows [0, R) = R1, [R, 2R) = R2;
//           score = (l2n(H[h] o R1[r]) . T[t] + l2n(H[t] o R2[r]) . T[h]) / 2 (each table row l2-normalised first),
//           loss = sum_pos softplus(-score) + sum_neg softplus(score).
//   DistMult u = l2n(ent)[e], w = l2n(rel)[r] (each by its flag), score = sum_d uh[d] w[d] ut[d],
//           loss = MEAN over the N = n_pos + n_neg labelled triples of softplus(-y score), y = +1 positives, -1 negatives
//           (batch.py:generate_triple_label_batch; the order of the labelled list does not enter the loss).
//
// One wave per positive and its k negatives; a lane holds columns 2 l and 2 l + 1 of every row.  The gradients w.r.t. the
// (table-)normalised rows go into the step engine's scratch, entity rows and relation copy 0, and the engine's apply phase
// (oea_triple_step_phase, OEA_PHASE_APPLY) takes them back through the table normalisation into the optimiser.  A row that the
// positive shares with its negatives is summed in registers and leaves the wave as ONE atomic row.
//
// HolE's three d x d sums per triple, with ds = dL/ds:
//   F[j] = sum_m rh[m] ut[(j + m) mod d]   = ds/duh[j]   (and s = uh . F)
//   C[j] = sum_m uh[m] ut[(m + j) mod d]   = ds/drh[j]   (= c)
//   G[j] = sum_m rh[m] uh[(j - m) mod d]   = ds/dut[j]
// The cyclic operand sits twice in LDS (x[0..d) x[0..d)), so that the index needs no modulo: every sum is
// out[j] = sum_m x[m] y[base_j + m] with a broadcast x and a sliding y.  A lane computes two adjacent outputs, so that each
// y it reads feeds two FMAs (four in the fused F / C loop).  Pass 1 computes F (the scores); pass 2, for groups whose
// hinge is active only, F and C in one loop and G in a second.
#include "common.h"
#include "row_ops.h"

#include <algorithm>

namespace {

using oea::flag_t;
using oea::grad_t;
using namespace oea::row;

constexpr int kMaxDim = 128;
constexpr int kWaves = 4;                 // waves per workgroup
constexpr int kY = 2 * kMaxDim + 8;       // a doubled operand + a zero tail the last iterations read
constexpr int kMaxBlocks = 2048;

struct SemArgs {
    const float *ent, *rel;
    int ld, dim;
    int64_t ent_half, rel_half;   // SimplE: E and R (the T / R2 halves start there)
    const int32_t *pos, *neg;
    int64_t n_pos;
    int k;
    float margin;
    int ent_l2n, rel_l2n;
    grad_t *ent_grad, *rel_grad;
    flag_t *ent_touched, *rel_touched;
    double *loss_accum;
    double inv_n;                 // DistMult: 1 / (n_pos + n_neg), the mean over the labelled triples
};

// ---- HolE ------------------------------------------------------------------------------------------------------------
struct HoleLds {
    float x[kMaxDim];     // rh
    float a[kMaxDim];     // uh
    float b2[kY];         // ut twice
    float ah2[kY];        // ah2[n] = uh[(-n) mod d], twice
    float buf[kMaxDim];   // flush_row
};

// (o0, o1) = (sum_m x[m] y[base + m], sum_m x[m] y[base + 1 + m]) over m < n4 (x zero from d on)
__device__ __forceinline__ float2 circ(const float *x, const float *y, int base, int n4) {
    const float *yp = y + base;
    float a0 = 0.f, a1 = 0.f, cur = yp[0];
#pragma unroll 2
    for (int m = 0; m < n4; m += 4) {
        const float4 xv = *reinterpret_cast<const float4 *>(x + m);
        const float y1 = yp[m + 1], y2 = yp[m + 2], y3 = yp[m + 3], y4 = yp[m + 4];
        a0 = fmaf(xv.x, cur, a0); a1 = fmaf(xv.x, y1, a1);
        a0 = fmaf(xv.y, y1, a0);  a1 = fmaf(xv.y, y2, a1);
        a0 = fmaf(xv.z, y2, a0);  a1 = fmaf(xv.z, y3, a1);
        a0 = fmaf(xv.w, y3, a0);  a1 = fmaf(xv.w, y4, a1);
        cur = y4;
    }
    return make_float2(a0, a1);
}

// F and C in one loop: both slide over y = b2 at the same base; x1 = rh, x2 = uh
__device__ __forceinline__ void circ_fc(const float *x1, const float *x2, const float *y, int base, int n4, float2 &f, float2 &c) {
    const float *yp = y + base;
    float f0 = 0.f, f1 = 0.f, c0 = 0.f, c1 = 0.f, cur = yp[0];
#pragma unroll 2
    for (int m = 0; m < n4; m += 4) {
        const float4 xa = *reinterpret_cast<const float4 *>(x1 + m);
        const float4 xb = *reinterpret_cast<const float4 *>(x2 + m);
        const float y1 = yp[m + 1], y2 = yp[m + 2], y3 = yp[m + 3], y4 = yp[m + 4];
        f0 = fmaf(xa.x, cur, f0); f1 = fmaf(xa.x, y1, f1); c0 = fmaf(xb.x, cur, c0); c1 = fmaf(xb.x, y1, c1);
        f0 = fmaf(xa.y, y1, f0);  f1 = fmaf(xa.y, y2, f1); c0 = fmaf(xb.y, y1, c0);  c1 = fmaf(xb.y, y2, c1);
        f0 = fmaf(xa.z, y2, f0);  f1 = fmaf(xa.z, y3, f1); c0 = fmaf(xb.z, y2, c0);  c1 = fmaf(xb.z, y3, c1);
        f0 = fmaf(xa.w, y3, f0);  f1 = fmaf(xa.w, y4, f1); c0 = fmaf(xb.w, y3, c0);  c1 = fmaf(xb.w, y4, c1);
        cur = y4;
    }
    f = make_float2(f0, f1);
    c = make_float2(c0, c1);
}

struct HoleRows {
    float2 uh, ut, rh;
    float n2;     // 1 / |l2n_table(rel)[r]| of the second normalisation
};

// the triple's rows, normalised, into the wave's LDS
__device__ __forceinline__ HoleRows hole_stage(const SemArgs &A, const int32_t *tr, int lane, HoleLds &L) {
    const int dim = A.dim;
    const float2 a = load2(A.ent + (int64_t)tr[0] * A.ld, dim, lane);
    const float2 b = load2(A.ent + (int64_t)tr[2] * A.ld, dim, lane);
    const float2 u = load2(A.rel + (int64_t)tr[1] * A.ld, dim, lane);
    HoleRows R;
    R.uh = scale2(a, inv_norm(a, A.ent_l2n));
    R.ut = scale2(b, inv_norm(b, A.ent_l2n));
    const float2 ur = scale2(u, inv_norm(u, A.rel_l2n));
    R.n2 = inv_norm(ur, 1);
    R.rh = scale2(ur, R.n2);
    __builtin_amdgcn_wave_barrier();          // the previous triple's reads are issued
    const int c = 2 * lane;
    *reinterpret_cast<float2 *>(L.x + c) = R.rh;
    *reinterpret_cast<float2 *>(L.a + c) = R.uh;
    const float uh2[2] = {R.uh.x, R.uh.y}, ut2[2] = {R.ut.x, R.ut.y};
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int cc = c + e;
        if (cc < dim) {
            L.b2[cc] = ut2[e];
            L.b2[cc + dim] = ut2[e];
            const int n0 = cc == 0 ? 0 : dim - cc;
            L.ah2[n0] = uh2[e];
            L.ah2[n0 + dim] = uh2[e];
        }
    }
    __builtin_amdgcn_wave_barrier();
    return R;
}

__global__ __launch_bounds__(64 * kWaves) void hole_kernel(SemArgs A) {
    __shared__ __attribute__((aligned(16))) HoleLds lds[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    HoleLds &L = lds[wave];
    for (int i = lane; i < kY; i += 64) { L.b2[i] = 0.f; L.ah2[i] = 0.f; }
    const int dim = A.dim, n4 = (dim + 3) & ~3, k = A.k;
    const int fbase = 2 * lane < dim ? 2 * lane : 0;                  // F, C: y = b2 at 2 l
    const int gbase = max(dim - 2 * lane - 1, 0);                     // G: y = ah2 at d - 2 l - 1 (outputs 2 l + 1, 2 l)
    const float inv_k = 1.f / (float)k;
    double loss_local = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * kWaves + wave; p < A.n_pos; p += (int64_t)gridDim.x * kWaves) {
        // pass 1: the scores
        float sig_pos = 0.f, sig_neg = 0.f;
        for (int q = 0; q <= k; ++q) {
            const int32_t *tr = q == 0 ? A.pos + 3 * p : A.neg + 3 * (p * k + q - 1);
            const HoleRows R = hole_stage(A, tr, lane, L);
            const float2 F = circ(L.x, L.b2, fbase, n4);
            const float sg = sigmoid_f(dot2(R.uh, F));
            if (q == 0) sig_pos = sg; else sig_neg += sg;
        }
        const float l = A.margin - sig_pos + sig_neg * inv_k;
        if (!(l > 0.f)) continue;                  // inactive hinge: no gradient, no row touched
        loss_local += (double)l;
        // pass 2: the gradients
        const int32_t *tp = A.pos + 3 * p;
        Slots<2> se;
        Slots<1> sr;
        se.set(0, tp[0]); se.set(1, tp[2]);
        sr.set(0, tp[1]);
        for (int q = 0; q <= k; ++q) {
            const int32_t *tr = q == 0 ? tp : A.neg + 3 * (p * k + q - 1);
            const HoleRows R = hole_stage(A, tr, lane, L);
            float2 F, C;
            circ_fc(L.x, L.a, L.b2, fbase, n4, F, C);
            const float2 Gr = circ(L.x, L.ah2, gbase, n4);
            const float2 G = make_float2(Gr.y, Gr.x);
            const float sg = sigmoid_f(dot2(R.uh, F));
            const float ds = q == 0 ? -sg * (1.f - sg) : sg * (1.f - sg) * inv_k;
            const float2 gr = scale2(C, ds);                                   // dL/drh
            const float pr = dot2(R.rh, gr);
            const float2 gu = make_float2((gr.x - R.rh.x * pr) * R.n2, (gr.y - R.rh.y * pr) * R.n2);
            se.add(tr[0], scale2(F, ds), A.ent_grad, A.ent_touched, A.ld, dim, lane, L.buf);
            se.add(tr[2], scale2(G, ds), A.ent_grad, A.ent_touched, A.ld, dim, lane, L.buf);
            sr.add(tr[1], gu, A.rel_grad, A.rel_touched, A.ld, dim, lane, L.buf);
        }
        se.flush(A.ent_grad, A.ent_touched, A.ld, dim, lane, L.buf);
        sr.flush(A.rel_grad, A.rel_touched, A.ld, dim, lane, L.buf);
    }
    oea::block_loss_add<kWaves>(loss_local, lane, wave, A.loss_accum);
}

// ---- SimplE ----------------------------------------------------------------------------------------------------------
// one calc(a, rho, w) = l2n(a o rho) . w term with its gradient: dc/dw = xh, dc/da = z o rho, dc/drho = z o a,
// z = (w - xh c) / |a o rho|
struct Term {
    float2 a, rho, w, xh;
    float n, c;
};
__device__ __forceinline__ Term simple_term(const SemArgs &A, int64_t ea, int64_t r, int64_t ew, int lane) {
    Term T;
    const float2 a = load2(A.ent + ea * A.ld, A.dim, lane), w = load2(A.ent + ew * A.ld, A.dim, lane);
    const float2 rho = load2(A.rel + r * A.ld, A.dim, lane);
    T.a = scale2(a, inv_norm(a, A.ent_l2n));
    T.w = scale2(w, inv_norm(w, A.ent_l2n));
    T.rho = scale2(rho, inv_norm(rho, A.rel_l2n));
    const float2 x = mul2(T.a, T.rho);
    T.n = inv_norm(x, 1);
    T.xh = scale2(x, T.n);
    T.c = dot2(T.xh, T.w);
    return T;
}

__global__ __launch_bounds__(64 * kWaves) void simple_kernel(SemArgs A) {
    __shared__ __attribute__((aligned(16))) float buf[kWaves][kMaxDim];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t E = A.ent_half, R = A.rel_half;
    const int k = A.k;
    double loss_local = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * kWaves + wave; p < A.n_pos; p += (int64_t)gridDim.x * kWaves) {
        const int32_t *tp = A.pos + 3 * p;
        // the positive's rows: H[h], T[t], H[t], T[h]; R1[r], R2[r]
        Slots<4> se;
        Slots<2> sr;
        se.set(0, tp[0]); se.set(1, E + tp[2]); se.set(2, tp[2]); se.set(3, E + tp[0]);
        sr.set(0, tp[1]); sr.set(1, R + tp[1]);
        for (int q = 0; q <= k; ++q) {
            const int32_t *tr = q == 0 ? tp : A.neg + 3 * (p * k + q - 1);
            const int64_t h = tr[0], r = tr[1], t = tr[2];
            const Term t1 = simple_term(A, h, r, E + t, lane);          // calc(H[h], R1[r], T[t])
            const Term t2 = simple_term(A, t, R + r, E + h, lane);      // calc(H[t], R2[r], T[h])
            const float score = 0.5f * (t1.c + t2.c);
            const float x = q == 0 ? -score : score;
            loss_local += (double)softplus_f(x);
            const float g = 0.5f * (q == 0 ? -sigmoid_f(x) : sigmoid_f(x));   // dL/dc of either term
            auto back = [&](const Term &T, int64_t ea, int64_t er, int64_t ew) {
                const float2 z = make_float2((T.w.x - T.xh.x * T.c) * T.n * g, (T.w.y - T.xh.y * T.c) * T.n * g);
                se.add(ea, mul2(z, T.rho), A.ent_grad, A.ent_touched, A.ld, A.dim, lane, buf[wave]);
                se.add(ew, scale2(T.xh, g), A.ent_grad, A.ent_touched, A.ld, A.dim, lane, buf[wave]);
                sr.add(er, mul2(z, T.a), A.rel_grad, A.rel_touched, A.ld, A.dim, lane, buf[wave]);
            };
            back(t1, h, r, E + t);
            back(t2, t, R + r, E + h);
        }
        se.flush(A.ent_grad, A.ent_touched, A.ld, A.dim, lane, buf[wave]);
        sr.flush(A.rel_grad, A.rel_touched, A.ld, A.dim, lane, buf[wave]);
    }
    oea::block_loss_add<kWaves>(loss_local, lane, wave, A.loss_accum);
}

// ---- DistMult --------------------------------------------------------------------------------------------------------
// s = sum_d uh w ut;  ds = dL/ds = -y sigmoid(-y s) / N;  dL/duh = ds (w o ut), dL/dw = ds (uh o ut), dL/dut = ds (uh o w).
// With h == t both halves land in the same slot.
__global__ __launch_bounds__(64 * kWaves) void distmult_kernel(SemArgs A) {
    __shared__ __attribute__((aligned(16))) float buf[kWaves][kMaxDim];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = A.k;
    const float inv_n = (float)A.inv_n;
    double loss_local = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * kWaves + wave; p < A.n_pos; p += (int64_t)gridDim.x * kWaves) {
        const int32_t *tp = A.pos + 3 * p;
        Slots<2> se;
        Slots<1> sr;
        se.set(0, tp[0]); se.set(1, tp[2]);
        sr.set(0, tp[1]);
        for (int q = 0; q <= k; ++q) {
            const int32_t *tr = q == 0 ? tp : A.neg + 3 * (p * k + q - 1);
            const int64_t h = tr[0], r = tr[1], t = tr[2];
            const float2 a = load2(A.ent + h * A.ld, A.dim, lane), b = load2(A.ent + t * A.ld, A.dim, lane);
            const float2 c = load2(A.rel + r * A.ld, A.dim, lane);
            const float2 uh = scale2(a, inv_norm(a, A.ent_l2n)), ut = scale2(b, inv_norm(b, A.ent_l2n));
            const float2 w = scale2(c, inv_norm(c, A.rel_l2n));
            const float2 hw = mul2(uh, w);
            const float score = dot2(hw, ut);
            const float x = q == 0 ? -score : score;                            // -y s
            loss_local += (double)softplus_f(x);
            const float ds = (q == 0 ? -sigmoid_f(x) : sigmoid_f(x)) * inv_n;
            se.add(h, scale2(mul2(w, ut), ds), A.ent_grad, A.ent_touched, A.ld, A.dim, lane, buf[wave]);
            se.add(t, scale2(hw, ds), A.ent_grad, A.ent_touched, A.ld, A.dim, lane, buf[wave]);
            sr.add(r, scale2(mul2(uh, ut), ds), A.rel_grad, A.rel_touched, A.ld, A.dim, lane, buf[wave]);
        }
        se.flush(A.ent_grad, A.ent_touched, A.ld, A.dim, lane, buf[wave]);
        sr.flush(A.rel_grad, A.rel_touched, A.ld, A.dim, lane, buf[wave]);
    }
    oea::block_loss_add<kWaves>(loss_local, lane, wave, A.loss_accum, A.inv_n);
}

}  // namespace

extern "C" {

int oea_semantic_step(int32_t model, float *ent, float *ent_acc, int64_t n_ent, float *rel, float *rel_acc, int64_t n_rel,
                      int32_t dim, int32_t ld, const int32_t *pos, int64_t n_pos, const int32_t *neg, int64_t n_neg,
                      const oea_step_cfg *cfg, void *step_workspace, double *loss_accum, void *stream) {
    if (model != OEA_SEMANTIC_HOLE && model != OEA_SEMANTIC_SIMPLE && model != OEA_SEMANTIC_DISTMULT) {
        oea::set_error("oea_semantic_step: unknown model %d", model);
        return OEA_EUNSUPPORTED;
    }
    OEA_REQUIRE(ent && rel && cfg && step_workspace && loss_accum, "null pointer");
    OEA_REQUIRE(n_pos >= 0 && (pos || n_pos == 0) && (neg || n_neg == 0), "pos / neg");
    if (cfg->opt_kind != OEA_OPT_SGD && cfg->opt_kind != OEA_OPT_ADAGRAD) {
        oea::set_error("oea_semantic_step: optimizer %d (SGD or Adagrad only)", cfg->opt_kind);
        return OEA_EUNSUPPORTED;
    }
    OEA_REQUIRE(cfg->opt_kind == OEA_OPT_SGD || (ent_acc && rel_acc), "Adagrad needs its two accumulators");
    OEA_REQUIRE(cfg->score_kind == OEA_SCORE_TRANSE && cfg->loss_kind >= OEA_LOSS_MARGIN && cfg->loss_kind <= OEA_LOSS_ALIGN,
                "cfg: score_kind OEA_SCORE_TRANSE (the model brings its own score and loss)");
    const int64_t k = cfg->neg_group_k;
    OEA_REQUIRE(k >= 1 && n_neg == k * n_pos, "neg_group_k = k >= 1 and n_neg == k n_pos (neg[p k .. p k + k) corrupt pos p)");
    OEA_REQUIRE(ld % 4 == 0, "ld % 4 == 0");
    OEA_REQUIRE(dim > 0 && dim <= ld, "0 < dim <= ld");
    if (dim > kMaxDim) {
        oea::set_error("oea_semantic_step: dim %d > %d", dim, kMaxDim);
        return OEA_EUNSUPPORTED;
    }
    if (model == OEA_SEMANTIC_SIMPLE)
        OEA_REQUIRE(n_ent % 2 == 0 && n_rel % 2 == 0, "SimplE: stacked tables, ent = [H; T] (2E rows), rel = [R1; R2] (2R rows)");
    hipStream_t st = oea::as_stream(stream);
    if (n_pos > 0) {
        SemArgs A;
        A.ent = ent; A.rel = rel; A.ld = ld; A.dim = dim;
        A.ent_half = model == OEA_SEMANTIC_SIMPLE ? n_ent / 2 : n_ent;
        A.rel_half = model == OEA_SEMANTIC_SIMPLE ? n_rel / 2 : n_rel;
        A.pos = pos; A.neg = neg; A.n_pos = n_pos; A.k = (int)k;
        A.margin = cfg->margin; A.ent_l2n = cfg->ent_l2_norm; A.rel_l2n = cfg->rel_l2_norm;
        oea::step_scratch_rows(step_workspace, n_ent, n_rel, ld, &A.ent_grad, &A.ent_touched, &A.rel_grad, &A.rel_touched);
        A.loss_accum = loss_accum;
        A.inv_n = 1.0 / (double)(n_pos + n_neg);
        const unsigned grid = (unsigned)std::min<int64_t>(oea::ceil_div(n_pos, kWaves), kMaxBlocks);
        if (model == OEA_SEMANTIC_HOLE) hole_kernel<<<grid, 64 * kWaves, 0, st>>>(A);
        else if (model == OEA_SEMANTIC_DISTMULT) distmult_kernel<<<grid, 64 * kWaves, 0, st>>>(A);
        else simple_kernel<<<grid, 64 * kWaves, 0, st>>>(A);
        OEA_CHECK_HIP(hipGetLastError());
    }
    // entity / relation rows: the step engine's optimiser on what the kernel put into its scratch
    return oea_triple_step_phase(ent, ent_acc, n_ent, rel, rel_acc, n_rel, dim, ld, nullptr, 0, nullptr, 0, cfg, step_workspace,
                                 loss_accum, OEA_PHASE_APPLY, stream);
}

}  // extern "C"
