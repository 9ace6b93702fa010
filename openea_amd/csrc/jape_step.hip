// jape_step.hip -- the triple step of JAPE (approaches/jape.py:59-84 of the reference):
//
//   u = l2n(ent)[e], w = l2n(rel)[r] (each by its flag), score = sum_d (uh + w - ut)[d]^2,
//   loss = sum_pos score - neg_alpha sum_neg score          (no hinge: the negatives' term has a negative weight)
//
// One wave per positive and its k negatives, as distmult_kernel of semantic_step.hip: a lane holds columns 2 l and 2 l + 1 of
// every row, the gradients w.r.t. the normalised rows go into the step engine's scratch (entity rows, relation copy 0) and the
// engine's apply phase takes them back through the table normalisation into the optimiser.  With c = +1 for the positive and
// -neg_alpha for a negative and x = uh + w - ut:  dL/duh = dL/dw = 2 c x,  dL/dut = -2 c x.  A row that the positive shares
// with its negatives is summed in registers; with h == t both halves land in one slot and cancel there.
#include "common.h"
#include "row_ops.h"

#include <algorithm>

namespace {

using oea::flag_t;
using oea::grad_t;
using namespace oea::row;

constexpr int kMaxDim = 128;
constexpr int kWaves = 4;
constexpr int kMaxBlocks = 2048;

struct JapeArgs {
    const float *ent, *rel;
    int ld, dim;
    const int32_t *pos, *neg;
    int64_t n_pos;
    int k;
    float neg_alpha;
    int ent_l2n, rel_l2n;
    grad_t *ent_grad, *rel_grad;
    flag_t *ent_touched, *rel_touched;
    double *loss_accum;
};

__global__ __launch_bounds__(64 * kWaves) void jape_kernel(JapeArgs A) {
    __shared__ __attribute__((aligned(16))) float buf[kWaves][kMaxDim];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = A.k;
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
            const float2 x = make_float2(uh.x + w.x - ut.x, uh.y + w.y - ut.y);
            const float coef = q == 0 ? 1.f : -A.neg_alpha;
            loss_local += (double)coef * (double)dot2(x, x);
            const float2 g = scale2(x, 2.f * coef);
            se.add(h, g, A.ent_grad, A.ent_touched, A.ld, A.dim, lane, buf[wave]);
            se.add(t, scale2(g, -1.f), A.ent_grad, A.ent_touched, A.ld, A.dim, lane, buf[wave]);
            sr.add(r, g, A.rel_grad, A.rel_touched, A.ld, A.dim, lane, buf[wave]);
        }
        se.flush(A.ent_grad, A.ent_touched, A.ld, A.dim, lane, buf[wave]);
        sr.flush(A.rel_grad, A.rel_touched, A.ld, A.dim, lane, buf[wave]);
    }
    oea::block_loss_add<kWaves>(loss_local, lane, wave, A.loss_accum);
}

}  // namespace

extern "C" {

int oea_jape_step(float *ent, float *ent_acc, int64_t n_ent, float *rel, float *rel_acc, int64_t n_rel, int32_t dim, int32_t ld,
                  const int32_t *pos, int64_t n_pos, const int32_t *neg, int64_t n_neg, float neg_alpha, const oea_step_cfg *cfg,
                  void *step_workspace, double *loss_accum, void *stream) {
    OEA_REQUIRE(ent && rel && cfg && step_workspace && loss_accum, "null pointer");
    OEA_REQUIRE(n_pos >= 0 && (pos || n_pos == 0) && (neg || n_neg == 0), "pos / neg");
    if (cfg->opt_kind != OEA_OPT_SGD && cfg->opt_kind != OEA_OPT_ADAGRAD) {
        oea::set_error("oea_jape_step: optimizer %d (SGD or Adagrad only)", cfg->opt_kind);
        return OEA_EUNSUPPORTED;
    }
    OEA_REQUIRE(cfg->opt_kind == OEA_OPT_SGD || (ent_acc && rel_acc), "Adagrad needs its two accumulators");
    OEA_REQUIRE(cfg->score_kind == OEA_SCORE_TRANSE && cfg->loss_kind >= OEA_LOSS_MARGIN && cfg->loss_kind <= OEA_LOSS_ALIGN,
                "cfg: score_kind OEA_SCORE_TRANSE (the step brings its own score and loss)");
    const int64_t k = cfg->neg_group_k;
    OEA_REQUIRE(k >= 1 && n_neg == k * n_pos, "neg_group_k = k >= 1 and n_neg == k n_pos (neg[p k .. p k + k) corrupt pos p)");
    OEA_REQUIRE(neg_alpha >= 0.f, "neg_alpha >= 0");          // false for a NaN as well
    OEA_REQUIRE(ld % 4 == 0, "ld % 4 == 0");
    OEA_REQUIRE(dim > 0 && dim <= ld, "0 < dim <= ld");
    if (dim > kMaxDim) {
        oea::set_error("oea_jape_step: dim %d > %d", dim, kMaxDim);
        return OEA_EUNSUPPORTED;
    }
    hipStream_t st = oea::as_stream(stream);
    if (n_pos > 0) {
        JapeArgs A;
        A.ent = ent; A.rel = rel; A.ld = ld; A.dim = dim;
        A.pos = pos; A.neg = neg; A.n_pos = n_pos; A.k = (int)k;
        A.neg_alpha = neg_alpha; A.ent_l2n = cfg->ent_l2_norm; A.rel_l2n = cfg->rel_l2_norm;
        oea::step_scratch_rows(step_workspace, n_ent, n_rel, ld, &A.ent_grad, &A.ent_touched, &A.rel_grad, &A.rel_touched);
        A.loss_accum = loss_accum;
        const unsigned grid = (unsigned)std::min<int64_t>(oea::ceil_div(n_pos, kWaves), kMaxBlocks);
        jape_kernel<<<grid, 64 * kWaves, 0, st>>>(A);
        OEA_CHECK_HIP(hipGetLastError());
    }
    return oea_triple_step_phase(ent, ent_acc, n_ent, rel, rel_acc, n_rel, dim, ld, nullptr, 0, nullptr, 0, cfg, step_workspace,
                                 loss_accum, OEA_PHASE_APPLY, stream);
}

}  // extern "C"
