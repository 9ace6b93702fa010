// ptranse_step.hip -- the training steps of IPTransE (approaches/iptranse.py of the reference).
//
//   train_loss     = margin(TransE, L2, one negative per positive)                                  (iptranse.py:158-165)
//                    + path_parm * sum_p (1 / w_p) relu(|x + y - r|^2 + margin - |x + y - r'|^2)     (iptranse.py:173-181)
//                    with x, y, r, r' rows of the (l2-normalised) relation table;
//   alignment_loss = sum_i w_i relu(|h + r - t|^2 + margin - |h' + r' - t'|^2)                      (iptranse.py:167-170).
//
// The triple half of train_loss is the step engine's own margin step (oea_triple_step_phase).  The path half never touches a
// table row per path: with Rn the normalised relation table and G = Rn Rn^T (R x R, L2-resident),
//   hinge argument = margin + (G[r,r] - G[r',r']) - 2 (G[x,r] + G[y,r]) + 2 (G[x,r'] + G[y,r'])
// and the gradient w.r.t. the normalised rows is linear in Rn: Gpath = A Rn for a sparse R x R coefficient matrix A to which an
// active pair adds ten scalars (c = path_parm / w):
//   A[x,r'] += 2c  A[x,r] -= 2c  A[y,r'] += 2c  A[y,r] -= 2c
//   A[r,x]  -= 2c  A[r,y] -= 2c  A[r,r]  += 2c  A[r',x] += 2c  A[r',y] += 2c  A[r',r'] -= 2c
// so a path batch costs O(paths) atomics on scalars + two small fp32-MFMA products (oea_gemm_tn_f32) instead of
// O(paths x dim) atomics on rows.  Four stages per step:
//   1  path_norm_kernel   Rn (zero-padded to Rp = 4 ceil(R / 4) rows) and its transpose; the id check of the batch
//      G = (Rn^T)^T (Rn^T)                                     [oea_gemm_tn_f32, reduction length ld]
//   2  path_kernel        one thread per path pair: six Gram lookups, the hinge, the loss, ten adds into A^T, flags
//   3  Gpath = (A^T)^T Rn                                      [oea_gemm_tn_f32, reduction length Rp]
//   4  path_scatter_kernel  flagged rows of Gpath into the step engine's relation scratch (copy 0) + touched flags; clears
//      A^T and the flags for the next step
// A^T accumulates in the scratch's own type (oea::grad_t: fp32 atomics, or int64 fixed point in the deterministic build, where
// it is converted to fp32 once in front of the product), so libopenea_hip_det.so gives the same bits run to run.
//
// The weighted pair step (the alignment epochs: a few steps every bp_freq epochs) is one wave per (pos, neg) pair.
#include "common.h"

#include <algorithm>

namespace {

using oea::flag_t;
using oea::grad_t;

constexpr int kMaxRel = 2048;             // A and G at 16 MB each
constexpr int kBlock = 256;

static int pad4(int64_t n) { return (int)((n + 3) / 4 * 4); }

struct PathWs {
    float *rn;          // [Rp, ld] normalised relation table, rows >= R and columns >= dim zero
    float *rnt;         // [ld, Rp] its transpose
    float *g;           // [Rp, Rp] Gram matrix
    grad_t *at;         // [Rp, Rp] A^T: at[j Rp + i] = A[i, j]; zero between steps
    float *atf;         // deterministic build: A^T as fp32 (the product's operand); else = at
    float *gpath;       // [Rp, ld] A Rn
    int32_t *ref;       // [Rp] relation referenced by an active pair; zero between steps
    float *gemm_ws;     // partial tiles of the two products
};

static size_t path_layout(int64_t n_rel, int32_t ld, void *base, PathWs *ws) {
    const size_t Rp = (size_t)pad4(n_rel);
    char *p = static_cast<char *>(base);
    size_t off = 0;
    auto take = [&](size_t bytes) { char *q = p ? p + off : nullptr; off += oea::align256(bytes); return q; };
    // A^T and the flags first: the region that has to be zero before the first step
    char *at = take(sizeof(grad_t) * Rp * Rp);
    char *ref = take(sizeof(int32_t) * Rp);
    char *rn = take(sizeof(float) * Rp * ld);
    char *rnt = take(sizeof(float) * Rp * ld);
    char *g = take(sizeof(float) * Rp * Rp);
    char *atf = oea::kDetScratch ? take(sizeof(float) * Rp * Rp) : at;
    char *gpath = take(sizeof(float) * Rp * ld);
    const size_t gw = std::max(oea_gemm_tn_workspace_floats(ld, (int32_t)Rp, (int32_t)Rp),
                               oea_gemm_tn_workspace_floats((int64_t)Rp, (int32_t)Rp, ld));
    char *gemm_ws = take(sizeof(float) * std::max<size_t>(gw, 1));
    if (ws) {
        ws->at = reinterpret_cast<grad_t *>(at); ws->ref = reinterpret_cast<int32_t *>(ref);
        ws->rn = reinterpret_cast<float *>(rn); ws->rnt = reinterpret_cast<float *>(rnt);
        ws->g = reinterpret_cast<float *>(g); ws->atf = reinterpret_cast<float *>(atf);
        ws->gpath = reinterpret_cast<float *>(gpath); ws->gemm_ws = reinterpret_cast<float *>(gemm_ws);
    }
    return off;
}

// stage 1: one wave per row of the padded table; the whole grid also walks the batch's ids once (err_flag 3 = a path id
// outside [0, n_rel): the path kernel then leaves the batch out)
__global__ __launch_bounds__(kBlock) void path_norm_kernel(const float *__restrict__ rel, int n_rel, int Rp, int dim, int ld, int l2n,
                                                          float *__restrict__ rn, float *__restrict__ rnt,
                                                          const int32_t *__restrict__ paths, const int32_t *__restrict__ neg_rel,
                                                          int64_t n, int32_t *err_flag) {
    const int lane = threadIdx.x & 63;
    const int r = (int)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (r < Rp) {
        const bool live = r < n_rel;
        float ss = 0.f;
        for (int c = lane; c < dim; c += 64) {
            const float v = live ? rel[(int64_t)r * ld + c] : 0.f;
            ss = fmaf(v, v, ss);
        }
        ss = oea::group_sum<64>(ss);
        const float inv = l2n ? rsqrtf(fmaxf(ss, 1e-12f)) : 1.f;
        for (int c = lane; c < ld; c += 64) {
            const float v = (live && c < dim) ? rel[(int64_t)r * ld + c] * inv : 0.f;
            rn[(int64_t)r * ld + c] = v;
            rnt[(int64_t)c * Rp + r] = v;
        }
    }
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int x = paths[3 * i], y = paths[3 * i + 1], q = paths[3 * i + 2], z = neg_rel[i];
        bad |= (unsigned)x >= (unsigned)n_rel || (unsigned)y >= (unsigned)n_rel || (unsigned)q >= (unsigned)n_rel ||
               (unsigned)z >= (unsigned)n_rel;
    }
    if (bad) *err_flag = 3;
}

// stage 2: one thread per path pair
__global__ __launch_bounds__(kBlock) void path_kernel(const float *__restrict__ g, int Rp, const int32_t *__restrict__ paths,
                                                     const int32_t *__restrict__ neg_rel, const float *__restrict__ weight, int64_t n,
                                                     float margin, float path_parm, grad_t *__restrict__ at, int32_t *__restrict__ ref,
                                                     double *loss_accum, const int32_t *err_flag) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double l = 0.0;
    if (i < n && *err_flag == 0) {
        const int64_t x = paths[3 * i], y = paths[3 * i + 1], r = paths[3 * i + 2], q = neg_rel[i];
        const float grr = g[r * Rp + r], gqq = g[q * Rp + q];
        const float gxr = g[x * Rp + r], gyr = g[y * Rp + r], gxq = g[x * Rp + q], gyq = g[y * Rp + q];
        const float h = margin + (grr - gqq) - 2.f * (gxr + gyr) + 2.f * (gxq + gyq);
        if (h > 0.f) {
            const float c = path_parm * (1.f / weight[i]);
            l = (double)(c * h);
            const float c2 = 2.f * c;
            auto add = [&](int64_t row, int64_t col, float v) { oea::grad_add(at + col * Rp + row, v); };   // A[row, col]
            add(x, q, c2); add(x, r, -c2);
            add(y, q, c2); add(y, r, -c2);
            add(r, x, -c2); add(r, y, -c2); add(r, r, c2);
            add(q, x, c2); add(q, y, c2); add(q, q, -c2);
            ref[x] = 1; ref[y] = 1; ref[r] = 1; ref[q] = 1;
        }
    }
    oea::block_loss_add<kBlock / 64>(oea::wave_sum_d(l), threadIdx.x & 63, threadIdx.x >> 6, loss_accum);
}

#ifdef OEA_DET_SCRATCH
__global__ __launch_bounds__(kBlock) void path_convert_kernel(const grad_t *__restrict__ at, float *__restrict__ atf, int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock)
        atf[i] = oea::grad_val(at[i]);
}
#endif

// stage 4: block b owns relation row b (b < Rp); the whole grid clears A^T
__global__ __launch_bounds__(kBlock) void path_scatter_kernel(const float *__restrict__ gpath, int n_rel, int Rp, int dim, int ld,
                                                             int32_t *__restrict__ ref, grad_t *__restrict__ at,
                                                             grad_t *__restrict__ rel_grad, flag_t *__restrict__ rel_touched) {
    const int r = (int)blockIdx.x;
    const int flagged = ref[r];
    __syncthreads();
    if (threadIdx.x == 0) ref[r] = 0;
    if (flagged && r < n_rel) {
        for (int c = threadIdx.x; c < dim; c += kBlock) oea::grad_add(rel_grad + (int64_t)r * ld + c, gpath[(int64_t)r * ld + c]);
        if (threadIdx.x == 0) rel_touched[r] = 1;
    }
    const int64_t total = (int64_t)Rp * Rp;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) at[i] = 0;
}

// ---- the weighted pair step: one wave per pair (pos i, neg i) ---------------------------------------------------------
struct PairArgs {
    const float *ent, *rel;
    int ld, dim;
    const int32_t *pos, *neg;
    const float *weight;
    int64_t n;
    float margin;
    int ent_l2n, rel_l2n;
    grad_t *ent_grad, *rel_grad;
    flag_t *ent_touched, *rel_touched;
    double *loss_accum;
};

__device__ __forceinline__ float row_inv_norm(const float *row, int dim, int lane, int on) {
    if (!on) return 1.f;
    float ss = 0.f;
    for (int c = lane; c < dim; c += 64) ss = fmaf(row[c], row[c], ss);
    return rsqrtf(fmaxf(oea::group_sum<64>(ss), 1e-12f));
}

__global__ __launch_bounds__(kBlock) void weighted_pair_kernel(PairArgs A) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int dim = A.dim;
    double loss_local = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * (kBlock / 64) + wave; p < A.n; p += (int64_t)gridDim.x * (kBlock / 64)) {
        const int32_t *tp = A.pos + 3 * p, *tn = A.neg + 3 * p;
        const int64_t id[6] = {tp[0], tp[1], tp[2], tn[0], tn[1], tn[2]};       // h r t | h' r' t'
        const float *row[6];
        float inv[6];
#pragma unroll
        for (int s = 0; s < 6; ++s) {
            const bool is_rel = s == 1 || s == 4;
            row[s] = (is_rel ? A.rel : A.ent) + id[s] * A.ld;
            inv[s] = row_inv_norm(row[s], dim, lane, is_rel ? A.rel_l2n : A.ent_l2n);
        }
        float sp = 0.f, sn = 0.f;
        for (int c = lane; c < dim; c += 64) {
            const float dp = row[0][c] * inv[0] + row[1][c] * inv[1] - row[2][c] * inv[2];
            const float dn = row[3][c] * inv[3] + row[4][c] * inv[4] - row[5][c] * inv[5];
            sp = fmaf(dp, dp, sp);
            sn = fmaf(dn, dn, sn);
        }
        sp = oea::group_sum<64>(sp);
        sn = oea::group_sum<64>(sn);
        const float w = A.weight[p];
        const float h = sp + A.margin - sn;
        if (!(h > 0.f)) continue;                  // inactive hinge: no gradient, no row touched
        loss_local += (double)(w * h);
        const float w2 = 2.f * w;
        for (int c = lane; c < dim; c += 64) {
            const float dp = w2 * (row[0][c] * inv[0] + row[1][c] * inv[1] - row[2][c] * inv[2]);
            const float dn = -w2 * (row[3][c] * inv[3] + row[4][c] * inv[4] - row[5][c] * inv[5]);
            oea::grad_add(A.ent_grad + id[0] * A.ld + c, dp);
            oea::grad_add(A.rel_grad + id[1] * A.ld + c, dp);
            oea::grad_add(A.ent_grad + id[2] * A.ld + c, -dp);
            oea::grad_add(A.ent_grad + id[3] * A.ld + c, dn);
            oea::grad_add(A.rel_grad + id[4] * A.ld + c, dn);
            oea::grad_add(A.ent_grad + id[5] * A.ld + c, -dn);
        }
        if (lane == 0) {
            A.ent_touched[id[0]] = 1; A.rel_touched[id[1]] = 1; A.ent_touched[id[2]] = 1;
            A.ent_touched[id[3]] = 1; A.rel_touched[id[4]] = 1; A.ent_touched[id[5]] = 1;
        }
    }
    oea::block_loss_add<kBlock / 64>(loss_local, lane, wave, A.loss_accum);
}

// ---- the epoch's path batches ----------------------------------------------------------------------------------------
struct SampleArgs {
    const int32_t *paths[2];     // [n_side, 3]
    const float *w[2];           // [n_side]
    const int32_t *rels[2];      // the KG's relation list
    uint32_t n[2], nr[2];
    int64_t P, num1;
    int steps;
    uint32_t k0, k1, epoch;
    int32_t *out_paths, *out_neg;
    float *out_w;
};

__global__ __launch_bounds__(kBlock) void path_sample_kernel(SampleArgs a) {
    const int64_t total = (int64_t)a.steps * a.P;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += (int64_t)gridDim.x * kBlock) {
        const uint32_t step = (uint32_t)(t / a.P);
        const int64_t j = t % a.P;
        const int side = j < a.num1 ? 0 : 1;
        const uint32_t i = (uint32_t)(side ? j - a.num1 : j);
        const uint4 key = oea::philox4x32_10(a.epoch, step, (uint32_t)side, 0u, a.k0, a.k1);
        const uint32_t src = oea::perm_index(i, a.n[side], key.x);
        const uint4 draw = oea::philox4x32_10(a.epoch, step, (uint32_t)side + 2u, i, a.k0, a.k1);
        const int32_t *p = a.paths[side] + 3 * (int64_t)src;
        a.out_paths[3 * t] = p[0];
        a.out_paths[3 * t + 1] = p[1];
        a.out_paths[3 * t + 2] = p[2];
        a.out_neg[t] = a.rels[side][__umulhi(draw.x, a.nr[side])];
        a.out_w[t] = a.w[side][src];
    }
}

static int check_step_cfg(const char *who, const oea_step_cfg *cfg) {
    if (cfg->l1 != 0) {
        oea::set_error("%s: loss_norm L1 (the reference asserts L2)", who);
        return OEA_EUNSUPPORTED;
    }
    if (cfg->opt_kind != OEA_OPT_SGD && cfg->opt_kind != OEA_OPT_ADAGRAD) {
        oea::set_error("%s: optimizer %d (SGD or Adagrad only)", who, cfg->opt_kind);
        return OEA_EUNSUPPORTED;
    }
    return OEA_OK;
}

static int check_path_shape(const char *who, int64_t n_rel, int32_t dim, int32_t ld) {
    OEA_REQUIRE(n_rel > 0, "n_rel > 0");
    if (n_rel > kMaxRel) {
        oea::set_error("%s: n_rel %lld > %d (A and G at 16 MB each)", who, (long long)n_rel, kMaxRel);
        return OEA_EUNSUPPORTED;
    }
    OEA_REQUIRE(ld % 4 == 0, "ld % 4 == 0");
    OEA_REQUIRE(dim > 0 && dim <= ld, "0 < dim <= ld");
    return OEA_OK;
}

}  // namespace

extern "C" {

size_t oea_path_workspace_bytes(int64_t n_rel, int32_t ld) {
    if (n_rel <= 0 || n_rel > kMaxRel || ld <= 0 || ld % 4 != 0) return 0;
    return path_layout(n_rel, ld, nullptr, nullptr);
}

int oea_path_grad(const float *rel, int64_t n_rel, int32_t dim, int32_t ld, const int32_t *paths, const int32_t *neg_rel,
                  const float *weight, int64_t n, float margin, float path_parm, int32_t rel_l2_norm, void *step_workspace,
                  int64_t n_ent, void *path_workspace, double *loss_accum, int32_t *err_flag, void *stream) {
    int rc = check_path_shape("oea_path_grad", n_rel, dim, ld);
    if (rc != OEA_OK) return rc;
    OEA_REQUIRE(rel && step_workspace && path_workspace && loss_accum && err_flag, "null pointer");
    OEA_REQUIRE(n >= 0 && n_ent >= 0 && (n == 0 || (paths && neg_rel && weight)), "paths / neg_rel / weight");
    if (n == 0) return OEA_OK;
    grad_t *ent_grad, *rel_grad;
    flag_t *ent_touched, *rel_touched;
    oea::step_scratch_rows(step_workspace, n_ent, n_rel, ld, &ent_grad, &ent_touched, &rel_grad, &rel_touched);
    PathWs ws;
    path_layout(n_rel, ld, path_workspace, &ws);
    const int Rp = pad4(n_rel);
    hipStream_t st = oea::as_stream(stream);
    path_norm_kernel<<<(unsigned)oea::ceil_div(Rp, kBlock / 64), kBlock, 0, st>>>(rel, (int)n_rel, Rp, dim, ld, rel_l2_norm, ws.rn,
                                                                                  ws.rnt, paths, neg_rel, n, err_flag);
    OEA_CHECK_HIP(hipGetLastError());
    rc = oea_gemm_tn_f32(ws.rnt, Rp, Rp, ws.rnt, Rp, Rp, ld, ws.g, Rp, ws.gemm_ws, stream);
    if (rc != OEA_OK) return rc;
    path_kernel<<<(unsigned)oea::ceil_div(n, kBlock), kBlock, 0, st>>>(ws.g, Rp, paths, neg_rel, weight, n, margin, path_parm, ws.at,
                                                                       ws.ref, loss_accum, err_flag);
    OEA_CHECK_HIP(hipGetLastError());
#ifdef OEA_DET_SCRATCH
    path_convert_kernel<<<(unsigned)std::min<int64_t>(oea::ceil_div((int64_t)Rp * Rp, kBlock), 1024), kBlock, 0, st>>>(
        ws.at, ws.atf, (int64_t)Rp * Rp);
    OEA_CHECK_HIP(hipGetLastError());
#endif
    rc = oea_gemm_tn_f32(ws.atf, Rp, Rp, ws.rn, ld, ld, Rp, ws.gpath, ld, ws.gemm_ws, stream);
    if (rc != OEA_OK) return rc;
    path_scatter_kernel<<<(unsigned)Rp, kBlock, 0, st>>>(ws.gpath, (int)n_rel, Rp, dim, ld, ws.ref, ws.at, rel_grad, rel_touched);
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

int oea_ptranse_step(float *ent, float *ent_acc, int64_t n_ent, float *rel, float *rel_acc, int64_t n_rel, int32_t dim, int32_t ld,
                     const int32_t *pos, int64_t n_pos, const int32_t *neg, int64_t n_neg, const int32_t *paths,
                     const int32_t *neg_rel, const float *weight, int64_t n_paths, float path_parm, const oea_step_cfg *cfg,
                     void *step_workspace, void *path_workspace, double *loss_accum, int32_t *err_flag, void *stream) {
    OEA_REQUIRE(ent && rel && cfg && step_workspace && loss_accum, "null pointer");
    int rc = check_step_cfg("oea_ptranse_step", cfg);
    if (rc != OEA_OK) return rc;
    rc = check_path_shape("oea_ptranse_step", n_rel, dim, ld);
    if (rc != OEA_OK) return rc;
    OEA_REQUIRE(cfg->score_kind == OEA_SCORE_TRANSE && cfg->loss_kind == OEA_LOSS_MARGIN, "cfg: TransE score, margin-based loss");
    OEA_REQUIRE(cfg->opt_kind == OEA_OPT_SGD || (ent_acc && rel_acc), "Adagrad needs its two accumulators");
    OEA_REQUIRE(n_pos >= 0 && n_neg == n_pos && (pos || n_pos == 0) && (neg || n_neg == 0), "pos / neg: pairs (pos i, neg i)");
    OEA_REQUIRE(n_paths >= 0 && (n_paths == 0 || (paths && neg_rel && weight && path_workspace && err_flag)),
                "paths / neg_rel / weight / path_workspace / err_flag");
    rc = oea_triple_step_phase(ent, ent_acc, n_ent, rel, rel_acc, n_rel, dim, ld, pos, n_pos, neg, n_neg, cfg, step_workspace,
                               loss_accum, OEA_PHASE_GRAD, stream);
    if (rc != OEA_OK) return rc;
    if (n_paths > 0) {
        rc = oea_path_grad(rel, n_rel, dim, ld, paths, neg_rel, weight, n_paths, cfg->margin, path_parm, cfg->rel_l2_norm,
                           step_workspace, n_ent, path_workspace, loss_accum, err_flag, stream);
        if (rc != OEA_OK) return rc;
    }
    return oea_triple_step_phase(ent, ent_acc, n_ent, rel, rel_acc, n_rel, dim, ld, pos, n_pos, neg, n_neg, cfg, step_workspace,
                                 loss_accum, OEA_PHASE_APPLY, stream);
}

int oea_path_sample_epoch(const int32_t *paths1, const float *weight1, int64_t n1, const int32_t *paths2, const float *weight2,
                          int64_t n2, const int32_t *rels1, int32_t n_rels1, const int32_t *rels2, int32_t n_rels2, int32_t steps,
                          uint64_t seed, uint32_t epoch, int32_t *out_paths, int32_t *out_neg_rel, float *out_weight, void *stream) {
    OEA_REQUIRE(steps > 0 && n1 >= 0 && n2 >= 0 && n1 + n2 < ((int64_t)1 << 31), "steps > 0, 0 <= n1, n2, n1 + n2 < 2^31");
    const int64_t P = (n1 + n2) / steps;
    if (P == 0) return OEA_OK;
    const int64_t num1 = (int64_t)((double)n1 / (double)(n1 + n2) * (double)P);      // iptranse.py:77
    const int64_t num2 = P - num1;
    OEA_REQUIRE(num1 <= n1 && num2 <= n2, "a step's sample is larger than its path list");
    OEA_REQUIRE(out_paths && out_neg_rel && out_weight, "null output");
    OEA_REQUIRE(num1 == 0 || (paths1 && weight1 && rels1 && n_rels1 > 0), "KG1: paths, weights and relation list");
    OEA_REQUIRE(num2 == 0 || (paths2 && weight2 && rels2 && n_rels2 > 0), "KG2: paths, weights and relation list");
    SampleArgs a;
    a.paths[0] = paths1; a.paths[1] = paths2; a.w[0] = weight1; a.w[1] = weight2; a.rels[0] = rels1; a.rels[1] = rels2;
    a.n[0] = (uint32_t)n1; a.n[1] = (uint32_t)n2; a.nr[0] = (uint32_t)n_rels1; a.nr[1] = (uint32_t)n_rels2;
    a.P = P; a.num1 = num1; a.steps = steps;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32) ^ 0x50415448u; a.epoch = epoch;      // "PATH": apart from the triple sampler's stream
    a.out_paths = out_paths; a.out_neg = out_neg_rel; a.out_w = out_weight;
    path_sample_kernel<<<(unsigned)std::min<int64_t>(oea::ceil_div((int64_t)steps * P, kBlock), 4096), kBlock, 0,
                         oea::as_stream(stream)>>>(a);
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

int oea_ptranse_epoch(float *ent, float *ent_acc, int64_t n_ent, float *rel, float *rel_acc, int64_t n_rel, int32_t dim, int32_t ld,
                      const int32_t *pos_all, const int64_t *offsets_host, int32_t steps, const int32_t *neg_buf,
                      const int32_t *path_buf, const int32_t *neg_rel_buf, const float *weight_buf, int64_t P, float path_parm,
                      const oea_step_cfg *cfg, void *step_workspace, void *path_workspace, double *loss_accum, int32_t *err_flag,
                      void *stream) {
    OEA_REQUIRE(offsets_host && steps >= 0 && P >= 0, "offsets_host, steps >= 0, P >= 0");
    OEA_REQUIRE(P == 0 || (path_buf && neg_rel_buf && weight_buf), "path buffers");
    for (int s = 0; s < steps; ++s) {
        const int64_t lo = offsets_host[s], n = offsets_host[s + 1] - lo;
        OEA_REQUIRE(n >= 0 && (n == 0 || (pos_all && neg_buf)), "offsets_host ascending; pos_all / neg_buf");
        const int rc = oea_ptranse_step(ent, ent_acc, n_ent, rel, rel_acc, n_rel, dim, ld, n ? pos_all + 3 * lo : nullptr, n,
                                        n ? neg_buf + 3 * lo : nullptr, n, P ? path_buf + 3 * (int64_t)s * P : nullptr,
                                        P ? neg_rel_buf + (int64_t)s * P : nullptr, P ? weight_buf + (int64_t)s * P : nullptr, P,
                                        path_parm, cfg, step_workspace, path_workspace, loss_accum, err_flag, stream);
        if (rc != OEA_OK) return rc;
    }
    return OEA_OK;
}

int oea_weighted_pair_step(float *ent, float *ent_acc, int64_t n_ent, float *rel, float *rel_acc, int64_t n_rel, int32_t dim,
                           int32_t ld, const int32_t *pos, const int32_t *neg, const float *weight, int64_t n,
                           const oea_step_cfg *cfg, void *step_workspace, double *loss_accum, void *stream) {
    OEA_REQUIRE(ent && rel && cfg && step_workspace && loss_accum, "null pointer");
    int rc = check_step_cfg("oea_weighted_pair_step", cfg);
    if (rc != OEA_OK) return rc;
    OEA_REQUIRE(cfg->score_kind == OEA_SCORE_TRANSE, "cfg: TransE score");
    OEA_REQUIRE(cfg->opt_kind == OEA_OPT_SGD || (ent_acc && rel_acc), "Adagrad needs its two accumulators");
    OEA_REQUIRE(ld % 4 == 0, "ld % 4 == 0");
    OEA_REQUIRE(dim > 0 && dim <= ld, "0 < dim <= ld");
    OEA_REQUIRE(n >= 0 && (n == 0 || (pos && neg && weight)), "pos / neg / weight");
    if (n > 0) {
        PairArgs A;
        A.ent = ent; A.rel = rel; A.ld = ld; A.dim = dim; A.pos = pos; A.neg = neg; A.weight = weight; A.n = n;
        A.margin = cfg->margin; A.ent_l2n = cfg->ent_l2_norm; A.rel_l2n = cfg->rel_l2_norm;
        oea::step_scratch_rows(step_workspace, n_ent, n_rel, ld, &A.ent_grad, &A.ent_touched, &A.rel_grad, &A.rel_touched);
        A.loss_accum = loss_accum;
        const unsigned grid = (unsigned)std::min<int64_t>(oea::ceil_div(n, kBlock / 64), 2048);
        weighted_pair_kernel<<<grid, kBlock, 0, oea::as_stream(stream)>>>(A);
        OEA_CHECK_HIP(hipGetLastError());
    }
    return oea_triple_step_phase(ent, ent_acc, n_ent, rel, rel_acc, n_rel, dim, ld, nullptr, 0, nullptr, 0, cfg, step_workspace,
                                 loss_accum, OEA_PHASE_APPLY, stream);
}

}  // extern "C"
