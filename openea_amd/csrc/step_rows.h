// step_rows.h -- what the translational step (triple_step.hip) and everything above one step (step_epochs.hip: the dense partition,
// the boundary-row exchange, the one-call epochs) both need, and nothing else:
//   * the step workspace (StepWs, ws_layout): the gradient scratch, its touched flags and the loss partials;
//   * a table row as lane-strided fragments (Row and its loaders) and the optimiser update of one row (apply_one_row);
//   * the sum of a step's loss partials by one wave (add_loss_partials_wave);
//   * the width ladders (for_row_width, for_width16, for_apply_width) and the two counts every user of a step's partials shares
//     (step_items, loss_partials);
//   * the host functions triple_step.hip defines once for both units (namespace oea, below).
// Included by those two units ONLY.  Kernels, row types and ladders live in an anonymous namespace (one copy per translation unit,
// as in nce_half.h); what only the single-GPU step uses -- Row4, the scoring helpers, the loss coefficients, apply_relation_row,
// triple_wave's buffer resources, wave_rule -- stays in triple_step.hip.
#pragma once
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "step_plan.h"

namespace oea {

// 16-lane groups for the optimiser kernels when the tables do not fit the caches (see launch_step).  ONE rule for apply_rows,
// part_apply_kernel and halo_apply_kernel, on the size of the WHOLE table: the group width decides the order of the row reductions,
// and the partitioned job must round like the single-GPU job (bit for bit in the fixed-point build).  OEA_APPLY_G16 = 0 / 1
// overrides the size rule; it is read here alone.
bool apply_g16(int64_t n_ent, int64_t n_rel, int32_t ld);

// oea_triple_step_phase with an epoch's gathered-sum plan (step_plan.h): step `plan_step` of the plan, whose positives start at row
// plan_first_pos of the epoch.  plan == nullptr: the plain step, which is what oea_triple_step_phase passes.
int step_phase_planned(float *ent, float *ent_acc, int64_t n_ent, float *rel, float *rel_acc, int64_t n_rel, int32_t dim, int32_t ld,
                       const int32_t *pos, int64_t n_pos, const int32_t *neg, int64_t n_neg, const oea_step_cfg *cfg, void *workspace,
                       double *loss_accum, int32_t phase, void *stream, const StepPlanView *plan, int plan_step, int64_t plan_first_pos);

}  // namespace oea

#define OEA_TRY_RC(...) do { const int _rc = (__VA_ARGS__); if (_rc != OEA_OK) return _rc; } while (0)

namespace {

using oea::align256;
using oea::group_sum;

using oea::flag_t;
using oea::grad_t;      // float, or int64 fixed point in the deterministic build (common.h)

struct StepWs {
    grad_t *ent_grad, *rel_grad;        // rel_grad: copy 0 of the relation scratch [n_rel][ld]
    grad_t *rel_extra;                  // copies 1 .. kRelCopies-1, [kRelCopies-1][n_rel][ld]
    int64_t rel_copy_stride;            // n_rel * ld
    flag_t *ent_touched, *rel_touched;  // 1 = row received gradient (same type as the gradients: one SUM all-reduce covers both)
    grad_t *nrm_grad, *nrm_extra;       // TransH normal vectors: copy 0 / copies 1.. (same shapes as the relation scratch)
    flag_t *nrm_touched;
    double *partials;                   // [kMaxBlocks]; the planned step's partials past kMaxBlocks lie BEFORE it (plan_partial)
    // layout: [ent_grad | rel_grad (copy 0) | nrm_grad (copy 0) | ent_touched | rel_touched | nrm_touched] is the
    // contiguous prefix that data-parallel ranks all-reduce (the extra copies are folded into copy 0 first);
    // [rel_extra | nrm_extra | planned partials kMaxBlocks .. kMaxPlanPartials - 1 | partials] follow.
    __device__ __forceinline__ grad_t *rel_copy(int64_t c) const {
        return c == 0 ? rel_grad : rel_extra + (c - 1) * rel_copy_stride;
    }
    __device__ __forceinline__ grad_t *nrm_copy(int64_t c) const {
        return c == 0 ? nrm_grad : nrm_extra + (c - 1) * rel_copy_stride;
    }
};
constexpr int kMaxBlocks = 4096;
// The planned step (triple_step.hip: wave_geometry) runs one 4-wave workgroup per 4 positives and leaves up to kMaxPlanPartials
// partials.  The workspace ends with the kMaxBlocks partials every step has; everything before them is zero between steps (the
// scratch, the flags -- tests/test_step_plan_gpu.py holds a step to it), so the planned step's partials past kMaxBlocks, which lie
// before them, are cleared by the block that adds them up (add_loss_partials_block).
constexpr int kMaxPlanPartials = 8192;
__host__ __device__ __forceinline__ double *plan_partial(const StepWs &ws, int b) {
    return ws.partials + (b < kMaxBlocks ? b : b - kMaxPlanPartials);
}
// Relation rows are few (a few hundred) and shared by the whole batch: with one scratch row per
// relation the hottest relation took ~750 same-address atomics per step (19 of 45 us, measured).
// The relation scratch is therefore replicated kRelCopies times; a work item adds into copy
// (item index % kRelCopies) and apply_rows sums the copies.
constexpr int kRelCopies = 16;

static size_t ws_layout(int64_t n_ent, int64_t n_rel, int32_t ld, void *base, StepWs *ws) {
    size_t off = 0;
    char *b = static_cast<char *>(base);
    auto take = [&](size_t bytes) { size_t o = off; off += align256(bytes); return b ? b + o : nullptr; };
    grad_t *eg = (grad_t *)take(sizeof(grad_t) * (size_t)n_ent * ld);
    grad_t *rg = (grad_t *)take(sizeof(grad_t) * (size_t)n_rel * ld);
    grad_t *ng = (grad_t *)take(sizeof(grad_t) * (size_t)n_rel * ld);
    flag_t *et = (flag_t *)take(sizeof(flag_t) * (size_t)n_ent);
    flag_t *rt = (flag_t *)take(sizeof(flag_t) * (size_t)n_rel);
    flag_t *nt = (flag_t *)take(sizeof(flag_t) * (size_t)n_rel);
    grad_t *rx = (grad_t *)take(sizeof(grad_t) * (size_t)n_rel * ld * (kRelCopies - 1));
    grad_t *nx = (grad_t *)take(sizeof(grad_t) * (size_t)n_rel * ld * (kRelCopies - 1));
    static_assert(sizeof(double) * (kMaxPlanPartials - kMaxBlocks) % 256 == 0, "plan_partial: the two partial ranges are contiguous");
    (void)take(sizeof(double) * (kMaxPlanPartials - kMaxBlocks));
    double *pp = (double *)take(sizeof(double) * kMaxBlocks);
    if (ws) {
        ws->rel_copy_stride = n_rel * (int64_t)ld; ws->ent_grad = eg; ws->rel_grad = rg; ws->rel_extra = rx;
        ws->ent_touched = et; ws->rel_touched = rt; ws->nrm_grad = ng; ws->nrm_extra = nx; ws->nrm_touched = nt; ws->partials = pp;
    }
    return off;
}

// ---- lane-strided row fragments ------------------------------------------------------------------
template <int G, int IT>
struct Row;                 // (below its loaders)

// TIGHT (G == 32 only): the dispatch gives ld > (IT - 1) * 32, so only the last fragment needs the bound.  Used by the
// grouped scoring kernel (18.8 vs 19.2 us at the 15K shape, 64 vs 75 us at the 100K shape); apply_rows is SLOWER with it
// (13.2 vs 11.3 us, 83 vs 64 us: the optimiser's three row streams schedule worse as unconditional loads) and keeps the bound.
template <int G, int IT, bool TIGHT = false>
__device__ __forceinline__ void load_row(const float *__restrict__ base, int ld, int lane, Row<G, IT> &r) {
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int c = it * G + lane;
        r.v[it] = ((TIGHT && G == 32 && it < IT - 1) || c < ld) ? base[c] : 0.f;
    }
}
// a row of the gradient scratch: raw elements (exact sums of the relation copies), then ONE conversion to fp32
template <int G, int IT>
__device__ __forceinline__ void load_grad_raw(const grad_t *__restrict__ base, int ld, int lane, grad_t (&q)[IT]) {
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int c = it * G + lane;
        q[it] = c < ld ? base[c] : (grad_t)0;
    }
}
template <int G, int IT>
__device__ __forceinline__ void load_grad_row(const grad_t *__restrict__ base, int ld, int lane, Row<G, IT> &r) {
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int c = it * G + lane;
        r.v[it] = c < ld ? oea::grad_val(base[c]) : 0.f;
    }
}
// Lane l of a G-lane group holds elements l, l + G, ... of a row: IT fragments of one scalar.  The members are what the optimiser
// asks of a row; Row4 (triple_step.hip) answers the same calls on float4 fragments.  s(it, j): scalar j of fragment it, whose
// first column is col(it, lane).  dot_partial adds its products in ascending order and the signed forms take the sign as a select:
// the order and the form that this layout's bits rest on.
template <int G, int IT>
struct Row {
    static constexpr int kLanes = G, kFrags = IT, kWidth = 1;
    float v[IT];
    __device__ __forceinline__ static int col(int it, int lane) { return it * G + lane; }
    __device__ __forceinline__ float s(int it, int) const { return v[it]; }
    __device__ __forceinline__ static void put(float *p, const float (&x)[1]) { *p = x[0]; }
    __device__ __forceinline__ static void zero(grad_t *p) { *p = 0; }
    __device__ __forceinline__ void load(const float *__restrict__ base, int ld, int lane) { load_row<G, IT>(base, ld, lane, *this); }
    __device__ __forceinline__ void load_grad(const grad_t *__restrict__ base, int ld, int lane) { load_grad_row<G, IT>(base, ld, lane, *this); }
    __device__ __forceinline__ float dot_partial(const Row &o) const {
        float p = 0.f;
#pragma unroll
        for (int it = 0; it < IT; ++it) p += v[it] * o.v[it];
        return p;
    }
    __device__ __forceinline__ void set_signed(const Row &o, bool neg) {
#pragma unroll
        for (int it = 0; it < IT; ++it) v[it] = neg ? -o.v[it] : o.v[it];
    }
    __device__ __forceinline__ void add_signed(const Row &o, bool neg) {
#pragma unroll
        for (int it = 0; it < IT; ++it) v[it] += neg ? -o.v[it] : o.v[it];
    }
    // += o, and the scratch row g it was loaded from cleared on the way
    __device__ __forceinline__ void add_and_clear(const Row &o, grad_t *g, int ld, int lane) {
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            v[it] += o.v[it];
            if (col(it, lane) < ld) zero(g + col(it, lane));
        }
    }
};

// pull the summed gradient of one row back through the normalisation, apply Adagrad / SGD, clear the scratch row.  F: Row or Row4.
// CLEAR = false: the gradient did not come from the scratch row (the planned optimiser's gathered sums): nothing to zero
template <bool CLEAR = true, class F>
__device__ __forceinline__ void apply_one_row(float *__restrict__ v, float *__restrict__ acc, grad_t *__restrict__ g,
                                              flag_t *__restrict__ touched_flag, int ld, int lane, int on,
                                              const oea_step_cfg &cfg, const F &rv, const F &rg, const F &ra) {
    float inv = 1.f, ydg = 0.f;
    if (on) {
        const float ss = group_sum<F::kLanes>(rv.dot_partial(rv));
        inv = rsqrtf(fmaxf(ss, 1e-12f));
        const float dot = group_sum<F::kLanes>(rv.dot_partial(rg)) * inv;       // y . g
        ydg = ss > 1e-12f ? dot : 0.f;
    }
#pragma unroll
    for (int it = 0; it < F::kFrags; ++it) {
        const int c = F::col(it, lane);
        if (c < ld) {
            float gv[F::kWidth], nv[F::kWidth];
#pragma unroll
            for (int j = 0; j < F::kWidth; ++j) gv[j] = rg.s(it, j);
            if (on) {
#pragma unroll
                for (int j = 0; j < F::kWidth; ++j) gv[j] = (gv[j] - rv.s(it, j) * inv * ydg) * inv;
            }
            if (cfg.opt_kind == OEA_OPT_ADAGRAD) {
                float a[F::kWidth];
#pragma unroll
                for (int j = 0; j < F::kWidth; ++j) a[j] = ra.s(it, j) + gv[j] * gv[j];
                F::put(acc + c, a);
#pragma unroll
                for (int j = 0; j < F::kWidth; ++j) nv[j] = rv.s(it, j) - cfg.lr * gv[j] / sqrtf(a[j]);
                F::put(v + c, nv);
            } else {
#pragma unroll
                for (int j = 0; j < F::kWidth; ++j) nv[j] = rv.s(it, j) - cfg.lr * gv[j];
                F::put(v + c, nv);
            }
            if (CLEAR) F::zero(g + c);
        }
    }
    if (CLEAR && lane == 0) *touched_flag = 0;
}

// The loss partials of the scoring kernel into *loss_accum, in a fixed order, by one wave (threads 0..63 of a block call it).
// (The planned optimiser has a whole block do it: add_loss_partials_block of triple_step.hip.)
__device__ __forceinline__ void add_loss_partials_wave(const StepWs &ws, int n_partials, double *__restrict__ loss_accum) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n_partials; i += 64) s += ws.partials[i];
    s = oea::wave_sum_d(s);
    if (threadIdx.x == 0) *loss_accum += s;
}

// work items of the GRAD kernel of a step = how many loss partials it leaves (one per workgroup of ceil(items / groups per block)):
// ONE rule for launch_step and for everything that adds the partials up afterwards (oea_part_apply, the one-call epochs; ADVICE
// r04: the partitioned epoch took "grouped" from neg_group_k alone and under-counted TransD's partials -- the printed loss only)
static int64_t step_items(const oea_step_cfg &cfg, int64_t n_pos, int64_t n_neg) {
    const bool transh = cfg.score_kind == OEA_SCORE_TRANSH, transd = cfg.score_kind == OEA_SCORE_TRANSD;
    const bool transh_grouped = transh && cfg.loss_kind != OEA_LOSS_MARGIN && (n_neg == 0 || cfg.neg_group_k > 0);
    const bool projected = transd || (transh && !transh_grouped);
    const bool grouped = transh_grouped || (!projected && cfg.neg_group_k > 0 && cfg.loss_kind != OEA_LOSS_MARGIN);
    return (grouped || cfg.loss_kind == OEA_LOSS_MARGIN) ? n_pos : n_pos + n_neg;
}

// how many loss partials the GRAD kernel of a step leaves: one per workgroup of 256 / G groups, G = 32 up to ld 128 and 64 beyond
// (for_row_width below), none when it scored nothing.  ONE count for launch_step's grid and for everything that adds the partials up
static int loss_partials(int32_t ld, int64_t n_items) {
    const int gpb = 256 / (ld <= 128 ? 32 : 64);
    return n_items > 0 ? (int)std::min<int64_t>(std::max<int64_t>(oea::ceil_div(n_items, gpb), 1), kMaxBlocks) : 0;
}

// The width ladders.  Each lists its rungs ONCE and hands them to f as std::integral_constant.
template <int V>
using int_c = std::integral_constant<int, V>;

// f(G, IT): G-lane groups with IT fragments per lane, by the row length.  ld > 1280: OEA_EUNSUPPORTED, nothing called.
// Measured and dropped (round 4, run r04f): 64-lane groups for 64 < ld <= 128 (one positive per wave, two fragments
// per lane): scoring kernel 17.8 -> 20.0 us at the 15K shape, 64.2 -> 60.4 us at the 100K shape, where the 64-lane optimiser
// kernel loses 18 us against the 16-lane one -- 3 % at best for a second instantiation of every kernel.
template <class F>
static int for_row_width(int32_t ld, F &&f) {
    if (ld <= 32) f(int_c<32>{}, int_c<1>{});
    else if (ld <= 64) f(int_c<32>{}, int_c<2>{});
    else if (ld <= 96) f(int_c<32>{}, int_c<3>{});
    else if (ld <= 128) f(int_c<32>{}, int_c<4>{});
    else if (ld <= 256) f(int_c<64>{}, int_c<4>{});
    else if (ld <= 512) f(int_c<64>{}, int_c<8>{});
    else if (ld <= 1280) f(int_c<64>{}, int_c<20>{});
    else { oea::set_error("ld %d > 1280 unsupported", ld); return OEA_EUNSUPPORTED; }
    return OEA_OK;
}

// f(IT): 16-lane groups (the optimiser kernels where apply_g16 says so, ld <= 128) with IT = ceil(ld / 16) fragments per lane
template <class F>
static void for_width16(int32_t ld, F &&f) {
    const int it16 = (ld + 15) / 16;
    if (it16 <= 2) f(int_c<2>{});
    else if (it16 <= 4) f(int_c<4>{});
    else if (it16 == 5) f(int_c<5>{});
    else if (it16 == 6) f(int_c<6>{});
    else if (it16 == 7) f(int_c<7>{});
    else f(int_c<8>{});
}

// 16-lane groups where apply_g16 says so, for_row_width's otherwise: the width of the optimiser kernels of the OWNED rows
// (part_apply_kernel, halo_apply_kernel) -- the single-GPU job's at this table size (launch_step: G == 32 is ld <= 128)
template <class F>
static int for_apply_width(int64_t n_ent, int64_t n_rel, int32_t ld, F &&f) {
    if (ld > 128 || !oea::apply_g16(n_ent, n_rel, ld)) return for_row_width(ld, f);
    for_width16(ld, [&](auto it) { f(int_c<16>{}, it); });
    return OEA_OK;
}

}  // namespace
