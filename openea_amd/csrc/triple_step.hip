// triple_step.hip -- fused translational step for gfx950.
//
// Replaces one session.run([triple_loss, triple_optimizer]) of the reference
// (models/basic_model.py:222-232): 6x tf.nn.embedding_lookup on l2_normalize(table)
// (basic_model.py:89-94, modules/base/initializers.py:26), the translational losses
// (modules/base/losses.py:15-73, approaches/bootea.py:197), TF autodiff through the gather
// and the normalisation, duplicate-row summation, and Adagrad / SGD
// (modules/base/optimizers.py:4-20).
//
// This file is ONE step on ONE GPU: a GRAD phase (a scoring kernel adds dL/d(normalised row) into the step workspace's gradient
// scratch with hardware atomics -- fp32, or int64 fixed point in the deterministic build -- raises the rows' touched flags and
// leaves one loss partial per workgroup) and an APPLY phase (an optimiser kernel pulls every touched row's sum back through the
// normalisation, (g - y (y.g)) / |v|, applies Adagrad / SGD / Adam / Adadelta and clears the scratch for the next step).
// The workspace, the row fragments (Row), apply_one_row and the width ladders are in step_rows.h, shared with step_epochs.hip,
// which holds everything above one step: the one-call epochs, the dense partition (part_*) and the boundary-row exchange (halo_*).
//
// Layout: a G-lane group (for_row_width: G = 32 for ld <= 128, else 64) owns one work item; lane l holds elements l, l+G, l+2G, ...
// of a row, so every load AND every atomic instruction of the group covers one contiguous 128-B / 256-B segment of a table row.
//
// Which kernel runs (launch_step, by the step's configuration):
//   GRAD   triple_projected        TransD, and TransH with margin pairs or free negative lists: one group per work item
//          triple_transh_grouped   TransH with a per-triple loss on the sampler's grouped negatives
//          triple_wave             TransE where wave_rule admits it (limited loss, both tables normalised, 1..10 grouped negatives,
//                                  ld <= 256, OEA_STEP_WAVE != 0): one WAVE per positive, scalar ids, buffer instructions
//          triple_grouped          every other TransE step with grouped negatives (neg[p*k+s] corrupts head or tail of pos p,
//                                  batch.py:89-119): one group per positive and its k negatives, (3+k) rows read and (3+k) rows of
//                                  atomics instead of 3(1+k), specialised on (loss kind, norm)
//          triple_generic          arbitrary (pos, neg) lists and the margin loss (pos i paired with neg i): one group per triple
//          fold_rel_copies_kernel  after a GRAD-only phase and in front of the dense optimisers: relation copies 1.. into copy 0
//   APPLY  apply_rows_dense        Adam / Adadelta (every row every step)
//          apply_step_plan         a planned step (below), in one launch
//          apply_rows              everything else: one group per table row, relation rows first; 16-lane groups where
//                                  oea::apply_g16 says the tables do not fit the caches
//          apply_normal_rows       TransH's normal vectors, after either of the above
// Where the plan comes in: oea_triple_epoch_range (step_epochs.hip) builds an epoch's gathered-sum plan (step_plan.h) where
// oea_step_plan_supported admits it -- wave_rule, SGD / Adagrad, the fp32 build, tables past the caches -- and hands it to
// oea::step_phase_planned.  triple_wave<.., PLAN = true> then stores each positive's two gradient rows into plan->contrib instead
// of adding them to the scratch, in the plan's relation order, and apply_step_plan sums them per entity row in batch order; both
// are built for kPlanInstance's row widths alone.  Every other entry point passes no plan.
//
// Algorithmic bytes per scored triple: 3 rows read + 3 rows of gradient = 24*d.
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "common.h"
#include "step_plan.h"
#include "step_rows.h"

namespace {

// ---- scoring helpers on Row fragments (step_rows.h) ------------------------------------------------
template <int G, int IT>
__device__ __forceinline__ float sumsq(const Row<G, IT> &r) {
    float s = 0.f;
#pragma unroll
    for (int it = 0; it < IT; ++it) s += r.v[it] * r.v[it];
    return group_sum<G>(s);
}
// y = l2_normalize(v) when `on` (tf.nn.l2_normalize: v * rsqrt(max(sum v^2, 1e-12)))
template <int G, int IT>
__device__ __forceinline__ void normalize(Row<G, IT> &r, int on) {
    if (!on) return;
    const float inv = rsqrtf(fmaxf(sumsq<G, IT>(r), 1e-12f));
#pragma unroll
    for (int it = 0; it < IT; ++it) r.v[it] *= inv;
}
template <int G, int IT>
__device__ __forceinline__ float score(const Row<G, IT> &yh, const Row<G, IT> &yr, const Row<G, IT> &yt, int l1,
                                       Row<G, IT> &delta) {
    float s = 0.f;
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const float d = yh.v[it] + yr.v[it] - yt.v[it];
        delta.v[it] = d;
        s += l1 ? fabsf(d) : d * d;
    }
    return group_sum<G>(s);
}
__device__ __forceinline__ float sgn(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }

// g = coef * ds/d(delta)
template <int G, int IT>
__device__ __forceinline__ void dscore(const Row<G, IT> &delta, float coef, int l1, Row<G, IT> &g) {
#pragma unroll
    for (int it = 0; it < IT; ++it) g.v[it] = l1 ? coef * sgn(delta.v[it]) : 2.f * coef * delta.v[it];
}
// SKIPZERO: elements whose gradient is exactly 0 issue no atomic (L1 norm: sgn(0); a per-element branch) -- the grouped
// kernel's L2 paths turn it off (a zero there is a measure-zero event and the branches cost more than the atomics)
template <int G, int IT, bool SKIPZERO = true>
__device__ __forceinline__ void atomic_row(grad_t *__restrict__ dst, int ld, int lane, const Row<G, IT> &g, float sign) {
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int c = it * G + lane;
        const float v = sign * g.v[it];
        if (((G == 32 && it < IT - 1) || c < ld) && (!SKIPZERO || v != 0.f)) oea::grad_add(dst + c, v);
    }
}

__device__ __forceinline__ float softplusf_(float x) { return x > 0.f ? x + log1pf(expf(-x)) : log1pf(expf(x)); }
__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// dL/ds and the loss term of ONE triple for the per-triple losses (not margin).
__device__ __forceinline__ void triple_coef_kind(int loss_kind, const oea_step_cfg &cfg, bool is_pos, float s, float &coef,
                                                 float &l) {
    coef = 0.f; l = 0.f;
    switch (loss_kind) {
    case OEA_LOSS_LIMITED:  // losses.py:53-55
        if (is_pos) { const float x = s - cfg.pos_margin; if (x > 0.f) { l = x; coef = 1.f; } }
        else { const float x = cfg.neg_margin - s; if (x > 0.f) { l = cfg.balance * x; coef = -cfg.balance; } }
        break;
    case OEA_LOSS_LOGISTIC:  // losses.py:70-72
        if (is_pos) { l = softplusf_(s); coef = sigmoidf_(s); }
        else { l = softplusf_(-s); coef = -sigmoidf_(-s); }
        break;
    case OEA_LOSS_POSITIVE:  // losses.py:38
        l = s; coef = 1.f;
        break;
    case OEA_LOSS_ALIGN:  // bootea.py:197: -log sigmoid(-s) = softplus(s)
        l = softplusf_(s); coef = sigmoidf_(s);
        break;
    default: break;
    }
}
__device__ __forceinline__ void triple_coef(const oea_step_cfg &cfg, bool is_pos, float s, float &coef, float &l) {
    triple_coef_kind(cfg.loss_kind, cfg, is_pos, s, coef, l);
}

__device__ __forceinline__ void block_loss_partial(double loss_local, double *partials) {
    // fixed reduction tree -> the partial is deterministic
    __shared__ double sred[4];
    const double w = oea::wave_sum_d(loss_local);
    if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = sred[0] + sred[1] + sred[2] + sred[3];
}

// ---- kernel 1b: arbitrary triple lists + margin pairs --------------------------------------------
template <int G, int IT>
__global__ __launch_bounds__(256) void triple_generic(
    const float *__restrict__ ent, const float *__restrict__ rel, int ld, const int32_t *__restrict__ pos,
    int64_t n_pos, const int32_t *__restrict__ neg, int64_t n_neg, oea_step_cfg cfg, StepWs ws) {
    const int lane = threadIdx.x % G;
    const int64_t grp = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int64_t ngrp = (int64_t)gridDim.x * blockDim.x / G;
    const bool margin = cfg.loss_kind == OEA_LOSS_MARGIN;
    const int64_t items = margin ? n_pos : n_pos + n_neg;
    double loss_local = 0.0;
    for (int64_t item = grp; item < items; item += ngrp) {
        const bool is_pos = margin || item < n_pos;
        const int32_t *tr = is_pos ? pos + 3 * item : neg + 3 * (item - n_pos);
        const int h = tr[0], r = tr[1], t = tr[2];
        Row<G, IT> yh, yr, yt, delta, g;
        load_row<G, IT>(ent + (int64_t)h * ld, ld, lane, yh);
        load_row<G, IT>(rel + (int64_t)r * ld, ld, lane, yr);
        load_row<G, IT>(ent + (int64_t)t * ld, ld, lane, yt);
        normalize<G, IT>(yh, cfg.ent_l2_norm);
        normalize<G, IT>(yr, cfg.rel_l2_norm);
        normalize<G, IT>(yt, cfg.ent_l2_norm);
        const float s = score<G, IT>(yh, yr, yt, cfg.l1, delta);
        float coef, l;
        if (margin) {
            // losses.py:15-27: sum relu(margin + s+ - s-), pos i paired with neg i
            const int32_t *tn = neg + 3 * item;
            const int nh = tn[0], nr = tn[1], nt = tn[2];
            Row<G, IT> zh, zr, zt, dn;
            load_row<G, IT>(ent + (int64_t)nh * ld, ld, lane, zh);
            load_row<G, IT>(rel + (int64_t)nr * ld, ld, lane, zr);
            load_row<G, IT>(ent + (int64_t)nt * ld, ld, lane, zt);
            normalize<G, IT>(zh, cfg.ent_l2_norm);
            normalize<G, IT>(zr, cfg.rel_l2_norm);
            normalize<G, IT>(zt, cfg.ent_l2_norm);
            const float sn = score<G, IT>(zh, zr, zt, cfg.l1, dn);
            const float x = cfg.margin + s - sn;
            if (x <= 0.f) continue;
            if (lane == 0) loss_local += (double)x;
            dscore<G, IT>(dn, -1.f, cfg.l1, g);
            atomic_row<G, IT>(ws.ent_grad + (int64_t)nh * ld, ld, lane, g, 1.f);
            atomic_row<G, IT>(ws.rel_copy(item % kRelCopies) + (int64_t)nr * ld, ld, lane, g, 1.f);
            atomic_row<G, IT>(ws.ent_grad + (int64_t)nt * ld, ld, lane, g, -1.f);
            if (lane == 0) { ws.ent_touched[nh] = 1.f; ws.ent_touched[nt] = 1.f; ws.rel_touched[nr] = 1.f; }
            coef = 1.f;
        } else {
            triple_coef(cfg, is_pos, s, coef, l);
            if (lane == 0) loss_local += (double)l;
            if (coef == 0.f) continue;
        }
        dscore<G, IT>(delta, coef, cfg.l1, g);
        atomic_row<G, IT>(ws.ent_grad + (int64_t)h * ld, ld, lane, g, 1.f);
        atomic_row<G, IT>(ws.rel_copy(item % kRelCopies) + (int64_t)r * ld, ld, lane, g, 1.f);
        atomic_row<G, IT>(ws.ent_grad + (int64_t)t * ld, ld, lane, g, -1.f);
        if (lane == 0) { ws.ent_touched[h] = 1.f; ws.ent_touched[t] = 1.f; ws.rel_touched[r] = 1.f; }
    }
    block_loss_partial(loss_local, ws.partials);
}

// ---- kernel 1a: one group per positive + its k negatives -------------------------------------------
// The k corrupted rows are requested KC at a time BEFORE any of them is consumed, so a group pays
// one memory latency per chunk instead of one per negative (the first version walked the
// negatives with a prefetch depth of one and was latency-bound: 38 us for 5,000 x 11 triples).
// score one (h, r, t) as an independent triple (entries of a grouped batch that are not corruptions of
// their positive): 3 gathers, 3 atomics.
template <int G, int IT>
__device__ __forceinline__ double score_independent(const float *__restrict__ ent, const float *__restrict__ rel, int ld,
                                                    int lane, int64_t item, int ch, int cr, int ct, bool is_pos,
                                                    const oea_step_cfg &cfg, const StepWs &ws, int lk, int l1) {
    Row<G, IT> zh, zr, zt, delta, g;
    load_row<G, IT>(ent + (int64_t)ch * ld, ld, lane, zh);
    load_row<G, IT>(rel + (int64_t)cr * ld, ld, lane, zr);
    load_row<G, IT>(ent + (int64_t)ct * ld, ld, lane, zt);
    normalize<G, IT>(zh, cfg.ent_l2_norm);
    normalize<G, IT>(zr, cfg.rel_l2_norm);
    normalize<G, IT>(zt, cfg.ent_l2_norm);
    const float s = score<G, IT>(zh, zr, zt, l1, delta);
    float coef, l;
    triple_coef_kind(lk, cfg, is_pos, s, coef, l);
    if (coef != 0.f) {
        dscore<G, IT>(delta, coef, l1, g);
        atomic_row<G, IT>(ws.ent_grad + (int64_t)ch * ld, ld, lane, g, 1.f);
        atomic_row<G, IT>(ws.rel_copy(item % kRelCopies) + (int64_t)cr * ld, ld, lane, g, 1.f);
        atomic_row<G, IT>(ws.ent_grad + (int64_t)ct * ld, ld, lane, g, -1.f);
        if (lane == 0) { ws.ent_touched[ch] = 1.f; ws.ent_touched[ct] = 1.f; ws.rel_touched[cr] = 1.f; }
    }
    return (double)l;
}

// The step is latency-bound (a few thousand short waves, ~1,800 instructions each), so the kernel is
// organised around DEPENDENT ROUND TRIPS, two per positive: (1) the ids -- the positive's three and
// its negatives' 3k, fetched by the lanes of the group in one coalesced load each and handed round
// with cross-lane reads; (2) every row the group needs, 3 + k gathers issued back to back.  The
// arithmetic after that is branch-free per negative so the k reduction chains interleave.
// Occupancy: a batch of 5,000 positives is 2,500 waves; at 2 waves/SIMD the chip holds 2,048, and the 452
// late-comers doubled the kernel's critical path (25.9 us).  Capping the registers at 3 waves/SIMD (a few
// spilled dwords for IT >= 2) lets every wave start at once: 19.4 us.
// Measured and dropped (gpurun_out r02f, same binary, env-selected): 4 waves / SIMD (<= 128 VGPRs, ~40 spill accesses)
// 20.1 vs 17.8 us at the 15K shape and 90 vs 65 us at the 100K shape; no per-element zero test in front of the atomics
// (100 fewer VALU instructions) 19.4 vs 17.8 us -- the test skips WHOLE rows often (a positive inside its margin with only
// tail-corrupted negatives active leaves gt all zero).
template <int G, int IT, int LOSS, int L1>
__global__ __launch_bounds__(256, (IT <= 4 ? 3 : 2)) void triple_grouped(
    const float *__restrict__ ent, const float *__restrict__ rel, int ld, const int32_t *__restrict__ pos,
    int64_t n_pos, const int32_t *__restrict__ neg, int k, oea_step_cfg cfg, StepWs ws) {
    constexpr int KC = IT <= 4 ? 10 : (IT <= 8 ? 4 : 2);      // negatives in flight: KC * IT row registers
    static_assert(3 * KC <= G, "ids of a chunk fit one register across the group");
    const int lane = threadIdx.x % G;
    const int64_t grp = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int64_t ngrp = (int64_t)gridDim.x * blockDim.x / G;
    // LOSS / L1 >= 0: the loss kind and the norm are compile-time constants (one compact code path per kind: with the
    // run-time switch every call site carried the exp / log1p expansions of the logistic losses, 12,000 instructions)
    const int lk = LOSS >= 0 ? LOSS : cfg.loss_kind;
    const int l1 = L1 >= 0 ? L1 : cfg.l1;
    double loss_local = 0.0;
    for (int64_t p = grp; p < n_pos; p += ngrp) {
        const int32_t *ng = neg + (int64_t)p * k * 3;
        // ---- round trip 1: ids -------------------------------------------------------------------------
        const int pid = lane < 3 ? pos[3 * p + lane] : 0;
        int nid = lane < 3 * min(KC, k) ? ng[lane] : 0;
        const int h = __shfl(pid, 0, G), r = __shfl(pid, 1, G), t = __shfl(pid, 2, G);
        Row<G, IT> yh, yr, yt, delta, g, gh, gr, gt;
        load_row<G, IT, true>(ent + (int64_t)h * ld, ld, lane, yh);
        load_row<G, IT, true>(rel + (int64_t)r * ld, ld, lane, yr);
        load_row<G, IT, true>(ent + (int64_t)t * ld, ld, lane, yt);
        double lsum = 0.0;
        bool any = false;
        for (int base = 0; base < k; base += KC) {
            if (base > 0) nid = lane < 3 * min(KC, k - base) ? ng[3 * base + lane] : 0;
            int ce[KC];                                                // the corrupted entity of slot j
            unsigned tailm = 0, okm = 0, slow = 0;                     // per-slot flags as bit masks (registers are tight)
            Row<G, IT> yc[KC];
            // ---- round trip 2: the corrupted rows (and, first time round, the positive's) ----------------
#pragma unroll
            for (int j = 0; j < KC; ++j) {
                const int ch = __shfl(nid, 3 * j, G), cr = __shfl(nid, 3 * j + 1, G), ct = __shfl(nid, 3 * j + 2, G);
                const bool valid = base + j < k;
                const bool tl = ch == h;                               // tail corrupted (or neg == pos): uses yh, yr
                const bool ok = valid && cr == r && (tl || ct == t);
                tailm |= tl ? 1u << j : 0u;
                okm |= ok ? 1u << j : 0u;
                slow |= (valid && !ok) ? 1u << j : 0u;                 // entries that are not corruptions of this positive
                ce[j] = valid ? (tl ? ct : ch) : h;
                load_row<G, IT, true>(ent + (int64_t)ce[j] * ld, ld, lane, yc[j]);
            }
            if (base == 0) {
                normalize<G, IT>(yh, cfg.ent_l2_norm);
                normalize<G, IT>(yr, cfg.rel_l2_norm);
                normalize<G, IT>(yt, cfg.ent_l2_norm);
                const float s = score<G, IT>(yh, yr, yt, l1, delta);
                float coef, l;
                triple_coef_kind(lk, cfg, true, s, coef, l);
                lsum = (double)l;
                dscore<G, IT>(delta, coef, l1, g);
#pragma unroll
                for (int it = 0; it < IT; ++it) { gh.v[it] = g.v[it]; gr.v[it] = g.v[it]; gt.v[it] = -g.v[it]; }
                any = coef != 0.f;
            }
            if (slow) {                                                // rare: one copy of the code, ids re-read across lanes
#pragma unroll 1
                for (int j = 0; j < KC; ++j)
                    if ((slow >> j) & 1u)
                        lsum += score_independent<G, IT>(ent, rel, ld, lane, p, __shfl(nid, 3 * j, G), __shfl(nid, 3 * j + 1, G),
                                                         __shfl(nid, 3 * j + 2, G), false, cfg, ws, lk, l1);
            }
            float sc[KC];
#pragma unroll
            for (int j = 0; j < KC; ++j) {                             // branch-free: k independent chains
                normalize<G, IT>(yc[j], cfg.ent_l2_norm);
                float s = 0.f;
#pragma unroll
                for (int it = 0; it < IT; ++it) {
                    const bool tl = (tailm >> j) & 1u;
                    const float a = tl ? yh.v[it] : yc[j].v[it], b = tl ? yc[j].v[it] : yt.v[it];
                    const float d = a + yr.v[it] - b;
                    yc[j].v[it] = d;                                    // the row is not needed again: keep delta in place
                    s += l1 ? fabsf(d) : d * d;
                }
                sc[j] = group_sum<G>(s);
            }
#pragma unroll
            for (int j = 0; j < KC; ++j) {
                if (!((okm >> j) & 1u)) continue;
                const bool tl = (tailm >> j) & 1u;
                float coef, l;
                triple_coef_kind(lk, cfg, false, sc[j], coef, l);
                lsum += (double)l;
                if (coef != 0.f) {
                    any = true;
                    dscore<G, IT>(yc[j], coef, l1, g);
                    if (tl) {
#pragma unroll
                        for (int it = 0; it < IT; ++it) { gh.v[it] += g.v[it]; gr.v[it] += g.v[it]; }
                    } else {
#pragma unroll
                        for (int it = 0; it < IT; ++it) { gr.v[it] += g.v[it]; gt.v[it] -= g.v[it]; }
                    }
                    atomic_row<G, IT>(ws.ent_grad + (int64_t)ce[j] * ld, ld, lane, g, tl ? -1.f : 1.f);
                    if (lane == 0) ws.ent_touched[ce[j]] = 1.f;
                }
            }
        }
        if (k <= 0) {       // no negatives: the positive alone
            normalize<G, IT>(yh, cfg.ent_l2_norm);
            normalize<G, IT>(yr, cfg.rel_l2_norm);
            normalize<G, IT>(yt, cfg.ent_l2_norm);
            const float s = score<G, IT>(yh, yr, yt, l1, delta);
            float coef, l;
            triple_coef_kind(lk, cfg, true, s, coef, l);
            lsum = (double)l;
            dscore<G, IT>(delta, coef, l1, g);
#pragma unroll
            for (int it = 0; it < IT; ++it) { gh.v[it] = g.v[it]; gr.v[it] = g.v[it]; gt.v[it] = -g.v[it]; }
            any = coef != 0.f;
        }
        if (any) {
            atomic_row<G, IT>(ws.ent_grad + (int64_t)h * ld, ld, lane, gh, 1.f);
            atomic_row<G, IT>(ws.rel_copy(p % kRelCopies) + (int64_t)r * ld, ld, lane, gr, 1.f);
            atomic_row<G, IT>(ws.ent_grad + (int64_t)t * ld, ld, lane, gt, 1.f);
            if (lane == 0) { ws.ent_touched[h] = 1.f; ws.ent_touched[t] = 1.f; ws.rel_touched[r] = 1.f; }
        }
        if (lane == 0) loss_local += lsum;
    }
    block_loss_partial(loss_local, ws.partials);
}

// ---- kernel 1a'', round 6: one WAVE per positive ----------------------------------------------------------------------------------------
// triple_grouped puts two positives on a wave (one per 32-lane half).  Everything that depends on the ids -- row addresses, "is this
// negative a tail or a head corruption", "is its hinge active" -- is then per-LANE state: 64-bit address arithmetic on the VALU for every
// row, ids handed round by ds_bpermute, every conditional atomic under its own exec mask (of its 2,900 instructions 1,100 are scalar
// bookkeeping, 220 of them s_nop), 168 registers = three waves per SIMD.  Here a wave owns ONE positive:
//   * ids arrive by SCALAR loads (the wave index is uniform: s_load_dwordx16 + x8 + x4 + x2 for the 30 ids of 10 negatives);
//   * rows move through BUFFER instructions: one resource per table, the row's byte offset in the instruction's scalar offset (one
//     s_mul_i32 per row), lane * 4 in the vector offset, fragment * 256 in the immediate -- no address arithmetic on the VALU at all.
//     The lanes whose column of the LAST fragment lies past the row's end carry an out-of-range vector offset for that fragment:
//     the addressing hardware returns 0 for their loads and drops their atomics -- no exec masks, no clamps, no selects;
//   * all control flow is wave-uniform (s_cbranch_scc / vcc): an inactive hinge skips its atomics without touching exec;
//   * the sampler corrupts ONE side per round (batch.py:101-107), so the k negatives of a positive are almost always all tail
//     corruptions or all head corruptions: one uniform test picks a select-free loop (tail: d = (h + r) - c with h + r computed
//     once; head: d = (c + r) - t), and gh == gr (tail) / gt == -gr (head) bit for bit, so ONE accumulator serves both rows.
//     Positives with mixed sides (the sampler's second round, ~0.3 %) take the same two round trips with the side per negative: one
//     uniform branch picks the expression, the negative's gradient goes to its own row and to the positive's row on the side it kept,
//     all through the scratch.  Positives with entries that are not corruptions of them at all (the sampler makes none) are scored as
//     1 + k independent triples (score_independent: the same loss and gradient, three rows per triple);
//   * lane-strided fragments of 64 columns: ceil(ld / 64) registers per row (2 at d = 100, packed-fp32 instructions) -> ~64 registers.
// The scalar unit is shared by the CU's four SIMDs (one instruction per cycle): the scalar work per positive (~250 instructions)
// matters as much as the vector work (~400).
// Arithmetic per element as in triple_grouped (normalise, a + r - b, hinge coefficients, accumulation in slot order); the row
// reductions run over 64 lanes instead of 32, so sums differ from it in the last bit (both are held to the oracle at 1e-4).
// LIMITED loss, both tables normalised, k <= 10, ld <= 256; everything else stays on triple_grouped.
#ifdef OEA_DET_SCRATCH
constexpr int kGradShift = 3;
#else
constexpr int kGradShift = 2;
#endif
constexpr unsigned kBufFlags = 0x00020000u;                       // raw buffer, 32-bit data format (gfx90a / gfx94x / gfx950)
// Resources span 2 GB from the table's base; row byte offsets (scalar offset) stay below 1 GB (launch rule), so an offset of 3 GB in the
// vector register is out of range whether or not the hardware counts the scalar offset in its range check, and the sum never wraps.
constexpr int kBufRecords = (int)0x80000000u;
constexpr int kBufOob = (int)0xC0000000u;

__device__ __forceinline__ void buf_grad_add(__amdgpu_buffer_rsrc_t rs, float v, int voff, int soff, int imm) {
#ifdef OEA_DET_SCRATCH
    const long long q = oea::to_fixed(v);
    const int vo = voff + imm;
    // s_nop 4: the hazard recogniser does not look inside inline assembly, and a VMEM instruction must not read a scalar register a
    // VALU instruction (v_readlane of a spilled scalar, v_readfirstlane) wrote fewer than 5 wait states earlier
    asm volatile("s_nop 4\n\tbuffer_atomic_add_x2 %0, %1, %2, %3 offen" ::"v"(q), "v"(vo), "s"(rs), "s"(soff) : "memory");
#else
    __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(v, rs, voff + imm, soff, 0);
#endif
}
__device__ __forceinline__ void buf_flag_set(__amdgpu_buffer_rsrc_t rs, int row) {       // every lane stores the same word: one request
#ifdef OEA_DET_SCRATCH
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
    const u32x2 one = {1u, 0u};
    __builtin_amdgcn_raw_buffer_store_b64(one, rs, 0, row * 8, 0);
#else
    __builtin_amdgcn_raw_buffer_store_b32(0x3f800000u, rs, 0, row * 4, 0);
#endif
}
// `vt` = this lane's vector offset for the LAST fragment: its column's byte offset where the column exists, kBufOob where it does not
// (>= num_records under either reading of the range check: the access reads 0 / the atomic is dropped)
template <int IT>
__device__ __forceinline__ void wave_load_row(__amdgpu_buffer_rsrc_t rs, int soff, int v4, int vt, Row<64, IT> &r) {
#pragma unroll
    for (int it = 0; it < IT; ++it)
        r.v[it] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, it < IT - 1 ? v4 + it * 256 : vt, soff, 0));
}
template <int IT>
__device__ __forceinline__ void wave_atomic_row(__amdgpu_buffer_rsrc_t rs, int soff, int vg, int vgt, const Row<64, IT> &g, float sign) {
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        if (it < IT - 1) buf_grad_add(rs, sign * g.v[it], vg, soff, it * (64 << kGradShift));
        else buf_grad_add(rs, sign * g.v[it], vgt, soff, 0);
    }
}
// one relation row of gradient into the scratch copy of positive `p`, and the row's touched flag
template <int IT>
__device__ __forceinline__ void wave_rel_row(const StepWs &ws, int dbg, int64_t p, int r, int row_g, int vg, int vgt, const Row<64, IT> &g) {
    const int copy = (int)(p % kRelCopies);
    grad_t *rgb = copy == 0 ? ws.rel_grad : ws.rel_extra + (copy - 1) * ws.rel_copy_stride;
    const __amdgpu_buffer_rsrc_t rs_rg = __builtin_amdgcn_make_buffer_rsrc(rgb, 0, (dbg & 1) ? 0 : kBufRecords, kBufFlags);
    const __amdgpu_buffer_rsrc_t rs_rt = __builtin_amdgcn_make_buffer_rsrc(ws.rel_touched, 0, (dbg & 4) ? 0 : kBufRecords, kBufFlags);
    wave_atomic_row<IT>(rs_rg, r * row_g, vg, vgt, g, 1.f);
    buf_flag_set(rs_rt, r);
}
__device__ __forceinline__ float uniform_f(float x) {       // a value every lane holds -> scalar register (uniform branches on it)
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, x)));
}

__device__ __forceinline__ double uniform_d(double x) {     // the same for a double: two scalar registers instead of a vector pair
    const unsigned long long b = __builtin_bit_cast(unsigned long long, x);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(b >> 32));
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// y = l2_normalize(v) with the sum of squares as a scalar (tf.nn.l2_normalize: v * rsqrt(max(sum v^2, 1e-12)))
template <int IT>
__device__ __forceinline__ void wave_normalize(Row<64, IT> &r) {
    float s = 0.f;
#pragma unroll
    for (int it = 0; it < IT; ++it) s += r.v[it] * r.v[it];
    const float inv = rsqrtf(fmaxf(oea::wave_sum_uniform(s), 1e-12f));
#pragma unroll
    for (int it = 0; it < IT; ++it) r.v[it] *= inv;
}

// PLAN (step_plan.h): the positive's two gradient rows A = gacc, B = gpos leave as PLAIN stores into contrib[2 p + {0, 1}] (the
// epoch's plan tells the optimiser kernel which entity rows add which of them, with which sign, in which order); only the relation
// row and the corrupted rows of active negatives still go through the atomic scratch.
// `order` (PLAN only; step_plan.h: rel_order of this step): wave slot q handles positive order[q] -- the step's positives in stable
// ascending order of relation id, so a workgroup's waves nearly always hold one relation -- and the relation rows of a workgroup are
// summed in LDS before the atomics.  Everything else is indexed by the positive's batch index as before.  nullptr: slot q handles
// positive q and every wave issues its own relation row (OEA_STEP_REL_ORDER=0).
// WPB: waves per workgroup of a PLAN launch (launch_wave: 4, or 8 under OEA_STEP_WAVE_BLOCK=512) -- the rows of the relation sum in
// LDS; without a plan the workgroup is whatever launch_grouped gives it and nothing is summed.
template <int IT, int L1, int KT, bool PLAN, int WPB = 8>
__global__ __launch_bounds__(PLAN ? WPB * 64 : 512, (IT <= 2 ? (KT == 10 ? 8 : 7) : 4)) void triple_wave(
    const float *__restrict__ ent, const float *__restrict__ rel, int ld, const int32_t *__restrict__ pos,
    int64_t n_pos, const int32_t *__restrict__ neg, int k, oea_step_cfg cfg, StepWs ws, int dbg, float *__restrict__ contrib,
    const uint32_t *__restrict__ pflags, const uint32_t *__restrict__ order) {
    constexpr int G = 64, KC = 10;
    if (KT > 0) k = KT;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wpb = blockDim.x >> 6;                                          // wave_geometry's block: 4 or 8 waves (PLAN: WPB)
    const int64_t nw = (int64_t)gridDim.x * wpb;
    const int row_b = ld * 4, row_g = ld << kGradShift;                       // bytes per table row / scratch row
    // dbg (OEA_STEP_WAVE_DBG, experiments only): bit 0 = an empty resource for the scratch (every atomic is issued and dropped), bit 1 =
    // empty resources for the tables (every row load is issued and returns 0), bit 2 = no touched flags
    const __amdgpu_buffer_rsrc_t rs_ent = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(ent), 0, (dbg & 2) ? 0 : kBufRecords, kBufFlags);
    const __amdgpu_buffer_rsrc_t rs_rel = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(rel), 0, (dbg & 2) ? 0 : kBufRecords, kBufFlags);
    const __amdgpu_buffer_rsrc_t rs_eg = __builtin_amdgcn_make_buffer_rsrc(ws.ent_grad, 0, (dbg & 1) ? 0 : kBufRecords, kBufFlags);
    const __amdgpu_buffer_rsrc_t rs_et = __builtin_amdgcn_make_buffer_rsrc(ws.ent_touched, 0, (dbg & 4) ? 0 : kBufRecords, kBufFlags);
    const int v4 = lane * 4, vg = lane << kGradShift;
    const int c_last = (IT - 1) * 64 + lane;                                  // this lane's column in the last fragment
    const int vt = c_last < ld ? c_last * 4 : kBufOob, vgt = c_last < ld ? c_last << kGradShift : kBufOob;
    const float c_neg = L1 ? -cfg.balance : -2.f * cfg.balance;               // dL/dd of an active negative = c_neg * (d or sgn d)
    double loss_local = 0.0;
    // one positive p on this wave.  Returns -1, or (only with an order) the relation whose row `gacc` is still to be added to the scratch
    auto score_positive = [&](int64_t p, Row<G, IT> &gacc) -> int {
        const int32_t *pp = pos + 3 * p;
        const int32_t *ng = neg + p * k * 3;
        const int h = pp[0], r = pp[1], t = pp[2];
        Row<G, IT> yh, yr, yt;
        wave_load_row<IT>(rs_ent, h * row_b, v4, vt, yh);
        wave_load_row<IT>(rs_rel, r * row_b, v4, vt, yr);
        wave_load_row<IT>(rs_ent, t * row_b, v4, vt, yt);
        int ids[3 * KC];
        if (KT == KC || k == KC) {                                      // constant offsets -> wide scalar loads
#pragma unroll
            for (int q = 0; q < 3 * KC; ++q) ids[q] = ng[q];
        } else {
#pragma unroll
            for (int q = 0; q < 3 * KC; ++q) ids[q] = q < 3 * k ? ng[q] : 0;
        }
        // every entry a corruption of this positive, and all on one side?
        unsigned bad = 0, xh = 0, xt = 0;
#pragma unroll
        for (int j = 0; j < KC; ++j)
            if (KT == KC || j < k) {
                const unsigned a = (unsigned)(ids[3 * j] ^ h), b = (unsigned)(ids[3 * j + 2] ^ t), c = (unsigned)(ids[3 * j + 1] ^ r);
                bad |= c | min(a, b);
                xh |= a;
                xt |= b;
            }
        if (bad) {                                                      // foreign entries (the sampler makes none): 1 + k independent triples
            double ls = score_independent<G, IT>(ent, rel, ld, lane, p, h, r, t, true, cfg, ws, OEA_LOSS_LIMITED, L1);
#pragma unroll 1
            for (int j = 0; j < k; ++j)
                ls += score_independent<G, IT>(ent, rel, ld, lane, p, ng[3 * j], ng[3 * j + 1], ng[3 * j + 2], false, cfg, ws, OEA_LOSS_LIMITED, L1);
            loss_local = uniform_d(loss_local + ls);
            return -1;
        }
        if (min(xh, xt)) {
            // Mixed sides (the sampler's second round draws with the other side's coin: ~0.3 % of positives).  The side is per NEGATIVE:
            // an entry that keeps the head is a tail corruption (a negative equal to its positive among them, as in the oracle).  The
            // same two round trips as below and the same expressions, with one wave-uniform branch per negative.
            unsigned tmask = 0;                                         // bit j: negative j is a tail corruption
            int ce[KC];
            Row<G, IT> yc[KC];
#pragma unroll
            for (int j = 0; j < KC; ++j)
                if (KT == KC || j < k) {
                    const int nh = ids[3 * j], nt = ids[3 * j + 2];
                    const bool tl = nh == h;
                    tmask |= tl ? 1u << j : 0u;
                    ce[j] = tl ? nt : nh;
                    wave_load_row<IT>(rs_ent, ce[j] * row_b, v4, vt, yc[j]);
                }
            asm volatile("" : "+s"(tmask));                             // (the sides live in this one register, not as ten conditions)
#pragma unroll
            for (int it = 0; it < IT; ++it)                             // (opaque: nothing below is common code with the one-sided path)
                asm volatile("" : "+v"(yh.v[it]), "+v"(yr.v[it]), "+v"(yt.v[it]));
            wave_normalize<IT>(yh);
            wave_normalize<IT>(yr);
            wave_normalize<IT>(yt);
            Row<G, IT> u, gpos;
            float sp = 0.f;
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                u.v[it] = yh.v[it] + yr.v[it];
                const float d = u.v[it] - yt.v[it];
                gpos.v[it] = d;
                sp += L1 ? fabsf(d) : d * d;
            }
            const float xp = oea::wave_sum_uniform(sp) - cfg.pos_margin;
            const bool cpos = xp > 0.f;
            float lsum = cpos ? xp : 0.f;
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                gpos.v[it] = cpos ? (L1 ? sgn(gpos.v[it]) : 2.f * gpos.v[it]) : 0.f;
                gacc.v[it] = gpos.v[it];
            }
            // No new accumulators: an active negative sends g to its own row AND to the positive's row on the side it kept (+g head /
            // -g tail), both through the scratch; gacc sums every g for the relation row alone.
            bool anyneg = false;
#pragma unroll
            for (int j = 0; j < KC; ++j)
                if (KT == KC || j < k) {
                    const bool tl = (tmask >> j) & 1u;
                    wave_normalize<IT>(yc[j]);
                    float s = 0.f;
                    if (tl) {
#pragma unroll
                        for (int it = 0; it < IT; ++it) {
                            const float d = u.v[it] - yc[j].v[it];      // (h + r) - t'
                            yc[j].v[it] = d;
                            s += L1 ? fabsf(d) : d * d;
                        }
                    } else {
#pragma unroll
                        for (int it = 0; it < IT; ++it) {
                            const float d = yc[j].v[it] + yr.v[it] - yt.v[it];   // (h' + r) - t
                            yc[j].v[it] = d;
                            s += L1 ? fabsf(d) : d * d;
                        }
                    }
                    const float xn = cfg.neg_margin - oea::wave_sum_uniform(s);
                    if (xn > 0.f) {
                        lsum += cfg.balance * xn;
                        anyneg = true;
                        Row<G, IT> g;
#pragma unroll
                        for (int it = 0; it < IT; ++it) {
                            g.v[it] = L1 ? c_neg * sgn(yc[j].v[it]) : c_neg * yc[j].v[it];
                            gacc.v[it] += g.v[it];
                        }
                        const int pe = tl ? h : t;
                        const float sign_c = tl ? -1.f : 1.f;
                        wave_atomic_row<IT>(rs_eg, ce[j] * row_g, vg, vgt, g, sign_c);
                        buf_flag_set(rs_et, ce[j]);
                        wave_atomic_row<IT>(rs_eg, pe * row_g, vg, vgt, g, -sign_c);
                        buf_flag_set(rs_et, pe);
                    }
                }
            // the positive's own term: the plan lists no row of a positive outside its rule (plan_emit_kernel gives them sentinel
            // keys), so both rows take the scratch and no contrib row is stored
            if (cpos) {
                wave_atomic_row<IT>(rs_eg, h * row_g, vg, vgt, gpos, 1.f);
                buf_flag_set(rs_et, h);
                wave_atomic_row<IT>(rs_eg, t * row_g, vg, vgt, gpos, -1.f);
                buf_flag_set(rs_et, t);
            }
            loss_local = uniform_d(loss_local + (double)lsum);
            if (!(cpos | anyneg)) return -1;
            if (PLAN && order) return r;                                // the relation row leaves with the workgroup's sum
            wave_rel_row<IT>(ws, dbg, p, r, row_g, vg, vgt, gacc);
            return -1;
        }
        // tail side or head side (k == 0: vacuously tails), each a copy of the code below with the side a compile-time constant.  With
        // the side a run-time value and the mixed-side block in the function, the compiler hoists the ten rows' sums of squares above
        // the side test -- ten more live registers -- and <2, 0, 10, *> spill 40 B per lane; as two copies they take 61 / 60 VGPRs
        auto one_sided = [&](auto side) -> int {
            constexpr bool tails = decltype(side)::value;
            int ce[KC];
            Row<G, IT> yc[KC];
#pragma unroll
            for (int j = 0; j < KC; ++j)
                if (KT == KC || j < k) {
                    ce[j] = tails ? ids[3 * j + 2] : ids[3 * j];
                    wave_load_row<IT>(rs_ent, ce[j] * row_b, v4, vt, yc[j]);
                }
            // ---- the positive ------------------------------------------------------------------------------------------------------
            wave_normalize<IT>(yh);
            wave_normalize<IT>(yr);
            wave_normalize<IT>(yt);
            Row<G, IT> u, gpos;
            int r_sum = -1;
            float sp = 0.f;
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                u.v[it] = yh.v[it] + yr.v[it];
                const float d = u.v[it] - yt.v[it];
                gpos.v[it] = d;
                sp += L1 ? fabsf(d) : d * d;
            }
            const float xp = oea::wave_sum_uniform(sp) - cfg.pos_margin;  // losses.py:53: relu(s+ - pos_margin)
            const bool cpos = xp > 0.f;
            float lsum = cpos ? xp : 0.f;
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                gpos.v[it] = cpos ? (L1 ? sgn(gpos.v[it]) : 2.f * gpos.v[it]) : 0.f;
                gacc.v[it] = gpos.v[it];
            }
            // ---- the negatives: scores first (k independent chains), then hinges in slot order -------------------------------------
            float sc[KC];
            if (tails) {
#pragma unroll
                for (int j = 0; j < KC; ++j)
                    if (KT == KC || j < k) {
                        wave_normalize<IT>(yc[j]);
                        float s = 0.f;
#pragma unroll
                        for (int it = 0; it < IT; ++it) {
                            const float d = u.v[it] - yc[j].v[it];          // (h + r) - t'
                            yc[j].v[it] = d;
                            s += L1 ? fabsf(d) : d * d;
                        }
                        sc[j] = oea::wave_sum_uniform(s);
                    }
            } else {
#pragma unroll
                for (int j = 0; j < KC; ++j)
                    if (KT == KC || j < k) {
                        wave_normalize<IT>(yc[j]);
                        float s = 0.f;
#pragma unroll
                        for (int it = 0; it < IT; ++it) {
                            const float d = yc[j].v[it] + yr.v[it] - yt.v[it];   // (h' + r) - t
                            yc[j].v[it] = d;
                            s += L1 ? fabsf(d) : d * d;
                        }
                        sc[j] = oea::wave_sum_uniform(s);
                    }
            }
            bool anyneg = false;
            const float sign_c = tails ? -1.f : 1.f;                        // d/d(corrupted row): -g (tail) / +g (head)
#pragma unroll
            for (int j = 0; j < KC; ++j)
                if (KT == KC || j < k) {
                    const float xn = cfg.neg_margin - sc[j];     // losses.py:54: balance * relu(neg_margin - s-)
                    if (xn > 0.f) {
                        lsum += cfg.balance * xn;
                        anyneg = true;
                        Row<G, IT> g;
#pragma unroll
                        for (int it = 0; it < IT; ++it) {
                            g.v[it] = L1 ? c_neg * sgn(yc[j].v[it]) : c_neg * yc[j].v[it];
                            gacc.v[it] += g.v[it];
                        }
                        wave_atomic_row<IT>(rs_eg, ce[j] * row_g, vg, vgt, g, sign_c);
                        buf_flag_set(rs_et, ce[j]);
                    }
                }
            // ---- the positive's rows: tail side gh = gr = gacc, gt = -gpos; head side gr = gacc, gt = -gacc, gh = gpos -----------------
            if (PLAN) {
                const __amdgpu_buffer_rsrc_t rs_cb = __builtin_amdgcn_make_buffer_rsrc(contrib, 0, kBufRecords, kBufFlags);
                const int so = (int)p * 2 * row_b;                          // rows 2 p (A) and 2 p + 1 (B), always written: the plan reads them
#pragma unroll
                for (int it = 0; it < IT; ++it) {
                    const int vo = it < IT - 1 ? v4 + it * 256 : vt;
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, gacc.v[it]), rs_cb, vo, so, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, gpos.v[it]), rs_cb, vo, so + row_b, 0);
                }
            }
            if (cpos | anyneg) {
                if (PLAN && order) r_sum = r;                               // the relation row leaves with the workgroup's sum below
                else wave_rel_row<IT>(ws, dbg, p, r, row_g, vg, vgt, gacc);
                // without a plan both rows go through the atomic scratch; with one only the rows the plan marks as hubs of this step
                const unsigned via_atomics = PLAN ? pflags[p] : 3u;         // bit 0: head row, bit 1: tail row
                const bool h_full = tails, t_full = !tails;                  // the row that receives the whole sum (the other: the positive's term)
                if ((via_atomics & 1u) && (h_full || cpos)) {
                    wave_atomic_row<IT>(rs_eg, h * row_g, vg, vgt, h_full ? gacc : gpos, 1.f);
                    buf_flag_set(rs_et, h);
                }
                if ((via_atomics & 2u) && (t_full || cpos)) {
                    wave_atomic_row<IT>(rs_eg, t * row_g, vg, vgt, t_full ? gacc : gpos, -1.f);
                    buf_flag_set(rs_et, t);
                }
            }
            loss_local = uniform_d(loss_local + (double)lsum);     // every lane holds it: kept in scalar registers across the next positive
            return r_sum;
        };
        return xh == 0 ? one_sided(std::true_type{}) : one_sided(std::false_type{});
    };
    if constexpr (!PLAN) {
        for (int64_t p = (int64_t)blockIdx.x * wpb + wv; p < n_pos; p += nw) {  // wave slot = positive, grid stride
            Row<G, IT> gacc;
            (void)score_positive(p, gacc);
        }
    } else {
        for (int64_t q0 = (int64_t)blockIdx.x * wpb; q0 < n_pos; q0 += nw) {    // uniform per workgroup: the barrier below is legal
            const int64_t q = q0 + wv;                                          // this wave's slot; its positive is order[q]
            Row<G, IT> gacc;
            const int r_sum = q < n_pos ? score_positive(order ? (int64_t)order[q] : q, gacc) : -1;
            if (!order) continue;                                               // batch order: every wave added its own relation row
            // Guideline "sum what shares a destination on chip": the workgroup's waves leave (relation, row) in LDS; the first wave
            // in wave order that holds a relation adds the rows of the later waves that hold it too, in wave order (equal relations
            // need not be adjacent), and issues ONE row of atomics and ONE flag for the group, into the scratch copy of its own
            // positive.  Waves past the end, waves inside both margins and waves that scored independent triples (their atomics
            // are done) bring "no row" (-1).  Any number of waves per workgroup: 4 with one slot each (wave_geometry), 4 that take
            // two slots each under OEA_STEP_WAVE_BLOCK=256 (every pass of this loop sums its own 4 rows), 8 under =512.
            __shared__ float s_row[WPB][IT][64];
            __shared__ int s_rel[WPB];
            // this lane's byte offset inside a 64-float fragment, taken from the register the row loads use and made opaque: the
            // LDS addresses are formed here, not hoisted out of the loop into registers the scoring code needs (measured: 9 spilled)
            int lb = v4;
            asm volatile("" : "+v"(lb));
            const auto at = [lb](auto *base) { return (decltype(base))((char *)base + lb); };
            if (lb == 0) s_rel[wv] = r_sum;
            if (r_sum >= 0) {
#pragma unroll
                for (int it = 0; it < IT; ++it) *at(&s_row[wv][it][0]) = gacc.v[it];
            }
            __syncthreads();
            if (r_sum >= 0) {
                const int held = lb < wpb * 4 ? *at(&s_rel[0]) : -1;         // lane w: the relation wave w holds
                bool first = true;
#pragma unroll
                for (int w = 0; w < WPB; ++w) first = first && !(w < wv && __builtin_amdgcn_readlane(held, w) == r_sum);
                if (first) {
#pragma unroll
                    for (int w = 1; w < WPB; ++w)
                        if (w > wv && __builtin_amdgcn_readlane(held, w) == r_sum) {
#pragma unroll
                            for (int it = 0; it < IT; ++it) gacc.v[it] += *at(&s_row[w][it][0]);
                        }
                    wave_rel_row<IT>(ws, dbg, order[q], r_sum, row_g, vg, vgt, gacc);
                }
            }
            if (q0 + nw < n_pos) __syncthreads();                       // the next pass writes the rows again
        }
    }
    // one partial per workgroup, fixed order
    __shared__ double sred[8];
    int lz = v4;                                                              // lane 0 by the register that is live anyway: with the
    if constexpr (PLAN) asm volatile("" : "+v"(lz));                          // combining loop `lane` itself was kept in scratch for this test
    if (lz == 0) sred[wv] = loss_local;
    __syncthreads();
    if (wv == 0 && lz == 0) {
        double s = 0.0;
        for (int w = 0; w < wpb; ++w) s += sred[w];
        *(PLAN ? plan_partial(ws, (int)blockIdx.x) : ws.partials + blockIdx.x) = s;
    }
}

// ---- TransH (approaches/bootea_transh.py:58-96) ---------------------------------------------------------------
// h' = h - (h.n) n, t' = t - (t.n) n with n = l2n(l2n(normal[r])); s = |h' + r - t'|.  With P = I - n n^T:
//   d/dh = P g,  d/dt = -P g,  d/dr = g,  d/dn = ((t.n) - (h.n)) g + (g.n) (t - h)        (g = dL/d delta).
// A separate, plainer kernel than triple_grouped (one group per positive and its k negatives, negatives
// two at a time): the TransE kernel's register budget stays what it is.
template <int G, int IT>
__device__ __forceinline__ float dot(const Row<G, IT> &a, const Row<G, IT> &b) {
    float s = 0.f;
#pragma unroll
    for (int it = 0; it < IT; ++it) s += a.v[it] * b.v[it];
    return group_sum<G>(s);
}
template <int G, int IT>
__device__ __forceinline__ void load_normal(const float *__restrict__ nrm, int r, int ld, int lane, Row<G, IT> &yn) {
    load_row<G, IT>(nrm + (int64_t)r * ld, ld, lane, yn);
    normalize<G, IT>(yn, 1);          // the variable is created with is_l2_norm=True ...
    normalize<G, IT>(yn, 1);          // ... and _calc normalises the looked-up row again
}
// one full triple with its own relation (positives of a batch without negatives; entries of a grouped batch
// that are not corruptions of their positive)
template <int G, int IT>
__device__ double transh_independent(const float *__restrict__ ent, const float *__restrict__ rel, int ld, int lane,
                                     int64_t item, int h, int r, int t, bool is_pos, const oea_step_cfg &cfg,
                                     const StepWs &ws) {
    Row<G, IT> yh, yr, yt, yn, delta, g;
    load_row<G, IT>(ent + (int64_t)h * ld, ld, lane, yh);
    load_row<G, IT>(rel + (int64_t)r * ld, ld, lane, yr);
    load_row<G, IT>(ent + (int64_t)t * ld, ld, lane, yt);
    load_normal<G, IT>(cfg.normal, r, ld, lane, yn);
    normalize<G, IT>(yh, cfg.ent_l2_norm);
    normalize<G, IT>(yr, cfg.rel_l2_norm);
    normalize<G, IT>(yt, cfg.ent_l2_norm);
    const float ah = dot<G, IT>(yh, yn), at = dot<G, IT>(yt, yn);
    float s = 0.f;
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const float d = (yh.v[it] - ah * yn.v[it]) + yr.v[it] - (yt.v[it] - at * yn.v[it]);
        delta.v[it] = d;
        s += cfg.l1 ? fabsf(d) : d * d;
    }
    s = group_sum<G>(s);
    float coef, l;
    triple_coef(cfg, is_pos, s, coef, l);
    if (coef != 0.f) {
        dscore<G, IT>(delta, coef, cfg.l1, g);
        const float gdn = dot<G, IT>(g, yn);
        Row<G, IT> pg, gn;
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            pg.v[it] = g.v[it] - gdn * yn.v[it];
            gn.v[it] = (at - ah) * g.v[it] + gdn * (yt.v[it] - yh.v[it]);
        }
        atomic_row<G, IT>(ws.ent_grad + (int64_t)h * ld, ld, lane, pg, 1.f);
        atomic_row<G, IT>(ws.ent_grad + (int64_t)t * ld, ld, lane, pg, -1.f);
        atomic_row<G, IT>(ws.rel_copy(item % kRelCopies) + (int64_t)r * ld, ld, lane, g, 1.f);
        atomic_row<G, IT>(ws.nrm_copy(item % kRelCopies) + (int64_t)r * ld, ld, lane, gn, 1.f);
        if (lane == 0) { ws.ent_touched[h] = 1.f; ws.ent_touched[t] = 1.f; ws.rel_touched[r] = 1.f; ws.nrm_touched[r] = 1.f; }
    }
    return (double)l;
}

template <int G, int IT>
__global__ __launch_bounds__(256) void triple_transh_grouped(
    const float *__restrict__ ent, const float *__restrict__ rel, int ld, const int32_t *__restrict__ pos,
    int64_t n_pos, const int32_t *__restrict__ neg, int k, oea_step_cfg cfg, StepWs ws) {
    const int lane = threadIdx.x % G;
    const int64_t grp = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int64_t ngrp = (int64_t)gridDim.x * blockDim.x / G;
    double loss_local = 0.0;
    for (int64_t p = grp; p < n_pos; p += ngrp) {
        const int h = pos[3 * p], r = pos[3 * p + 1], t = pos[3 * p + 2];
        const int32_t *ng = neg + (int64_t)p * k * 3;
        Row<G, IT> yh, yr, yt, yn, ph, pt, g, gh, gr, gt, gn;
        load_row<G, IT>(ent + (int64_t)h * ld, ld, lane, yh);
        load_row<G, IT>(rel + (int64_t)r * ld, ld, lane, yr);
        load_row<G, IT>(ent + (int64_t)t * ld, ld, lane, yt);
        load_normal<G, IT>(cfg.normal, r, ld, lane, yn);
        normalize<G, IT>(yh, cfg.ent_l2_norm);
        normalize<G, IT>(yr, cfg.rel_l2_norm);
        normalize<G, IT>(yt, cfg.ent_l2_norm);
        const float ah = dot<G, IT>(yh, yn), at = dot<G, IT>(yt, yn);
        float s = 0.f;
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            ph.v[it] = yh.v[it] - ah * yn.v[it];
            pt.v[it] = yt.v[it] - at * yn.v[it];
            const float d = ph.v[it] + yr.v[it] - pt.v[it];
            g.v[it] = d;
            s += cfg.l1 ? fabsf(d) : d * d;
        }
        s = group_sum<G>(s);
        float coef, l;
        triple_coef(cfg, true, s, coef, l);
        double lsum = (double)l;
        bool any = coef != 0.f;
        {
            Row<G, IT> d0 = g;
            dscore<G, IT>(d0, coef, cfg.l1, g);
            const float gdn = dot<G, IT>(g, yn);
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                const float pg = g.v[it] - gdn * yn.v[it];
                gh.v[it] = pg; gt.v[it] = -pg; gr.v[it] = g.v[it];
                gn.v[it] = (at - ah) * g.v[it] + gdn * (yt.v[it] - yh.v[it]);
            }
        }
        for (int j0 = 0; j0 < k; j0 += 2) {
            int ch[2], cr[2], ct[2];
            Row<G, IT> yc[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int j = j0 + u < k ? j0 + u : j0;
                ch[u] = ng[3 * j]; cr[u] = ng[3 * j + 1]; ct[u] = ng[3 * j + 2];
                load_row<G, IT>(ent + (int64_t)((ch[u] == h) ? ct[u] : ch[u]) * ld, ld, lane, yc[u]);
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (j0 + u >= k) continue;
                const bool tail = ch[u] == h;
                if (!(cr[u] == r && (tail || ct[u] == t))) {              // not a corruption of this positive
                    lsum += transh_independent<G, IT>(ent, rel, ld, lane, p, ch[u], cr[u], ct[u], false, cfg, ws);
                    continue;
                }
                const int ce = tail ? ct[u] : ch[u];
                normalize<G, IT>(yc[u], cfg.ent_l2_norm);
                const float ac = dot<G, IT>(yc[u], yn);
                Row<G, IT> delta;
                s = 0.f;
#pragma unroll
                for (int it = 0; it < IT; ++it) {
                    const float pc = yc[u].v[it] - ac * yn.v[it];
                    const float d = tail ? ph.v[it] + yr.v[it] - pc : pc + yr.v[it] - pt.v[it];
                    delta.v[it] = d;
                    s += cfg.l1 ? fabsf(d) : d * d;
                }
                s = group_sum<G>(s);
                triple_coef(cfg, false, s, coef, l);
                lsum += (double)l;
                if (coef == 0.f) continue;
                any = true;
                dscore<G, IT>(delta, coef, cfg.l1, g);
                const float gdn = dot<G, IT>(g, yn);
                Row<G, IT> pg;
#pragma unroll
                for (int it = 0; it < IT; ++it) {
                    pg.v[it] = g.v[it] - gdn * yn.v[it];
                    gr.v[it] += g.v[it];
                    if (tail) {
                        gh.v[it] += pg.v[it];
                        gn.v[it] += (ac - ah) * g.v[it] + gdn * (yc[u].v[it] - yh.v[it]);
                    } else {
                        gt.v[it] -= pg.v[it];
                        gn.v[it] += (at - ac) * g.v[it] + gdn * (yt.v[it] - yc[u].v[it]);
                    }
                }
                atomic_row<G, IT>(ws.ent_grad + (int64_t)ce * ld, ld, lane, pg, tail ? -1.f : 1.f);
                if (lane == 0) ws.ent_touched[ce] = 1.f;
            }
        }
        if (any) {
            atomic_row<G, IT>(ws.ent_grad + (int64_t)h * ld, ld, lane, gh, 1.f);
            atomic_row<G, IT>(ws.ent_grad + (int64_t)t * ld, ld, lane, gt, 1.f);
            atomic_row<G, IT>(ws.rel_copy(p % kRelCopies) + (int64_t)r * ld, ld, lane, gr, 1.f);
            atomic_row<G, IT>(ws.nrm_copy(p % kRelCopies) + (int64_t)r * ld, ld, lane, gn, 1.f);
            if (lane == 0) { ws.ent_touched[h] = 1.f; ws.ent_touched[t] = 1.f; ws.rel_touched[r] = 1.f; ws.nrm_touched[r] = 1.f; }
        }
        if (lane == 0) loss_local += lsum;
    }
    block_loss_partial(loss_local, ws.partials);
}

// ---- projected scores, one group per work item (models/trans/transh.py:16-51, models/trans/transd.py:16-57) ------
// The plain ModelFamily members: margin loss on pairs (pos i, neg i) or a per-triple loss on arbitrary lists, rows
// projected before the translation.
//   TransH  h' = h - (h.n) n                        n = l2n(l2n(normal[r]))            (transh.py:48-51)
//   TransD  h' = l2n(h + (h.hp) rp)                 hp = ent_transfer[h], rp = rel_transfer[r]  (transd.py:56-57)
// TransD keeps its transfer vectors in the SAME tables, rows [base, base + n): the gradient scratch, the exchange
// and apply_rows treat them like any other row (same l2_norm flag, same optimiser -- transd.py:16-24).
// mode 0: score only; 1: score + gradient with the given dL/ds; 2: dL/ds from the per-triple loss (returns it in l).
template <int G, int IT>
__device__ float transd_triple(const float *__restrict__ ent, const float *__restrict__ rel, int ld, int lane,
                               int64_t item, int h, int r, int t, bool is_pos, const oea_step_cfg &cfg,
                               const StepWs &ws, int mode, float coef, float &l) {
    const int64_t eb = cfg.ent_transfer_base, rb = cfg.rel_transfer_base;
    Row<G, IT> yh, yt, yr, hp, tp, rp, H, T, g;
    load_row<G, IT>(ent + (int64_t)h * ld, ld, lane, yh);
    load_row<G, IT>(ent + (int64_t)t * ld, ld, lane, yt);
    load_row<G, IT>(rel + (int64_t)r * ld, ld, lane, yr);
    load_row<G, IT>(ent + (eb + h) * ld, ld, lane, hp);
    load_row<G, IT>(ent + (eb + t) * ld, ld, lane, tp);
    load_row<G, IT>(rel + (rb + r) * ld, ld, lane, rp);
    normalize<G, IT>(yh, cfg.ent_l2_norm);
    normalize<G, IT>(yt, cfg.ent_l2_norm);
    normalize<G, IT>(yr, cfg.rel_l2_norm);
    normalize<G, IT>(hp, cfg.ent_l2_norm);
    normalize<G, IT>(tp, cfg.ent_l2_norm);
    normalize<G, IT>(rp, cfg.rel_l2_norm);
    const float ah = dot<G, IT>(yh, hp), at = dot<G, IT>(yt, tp);
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        H.v[it] = yh.v[it] + ah * rp.v[it];
        T.v[it] = yt.v[it] + at * rp.v[it];
    }
    const float ssh = sumsq<G, IT>(H), sst = sumsq<G, IT>(T);
    const float ih = rsqrtf(fmaxf(ssh, 1e-12f)), itl = rsqrtf(fmaxf(sst, 1e-12f));
    float s = 0.f;
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        H.v[it] *= ih;
        T.v[it] *= itl;
        const float d = H.v[it] + yr.v[it] - T.v[it];
        g.v[it] = d;
        s += cfg.l1 ? fabsf(d) : d * d;
    }
    s = group_sum<G>(s);
    l = 0.f;
    if (mode == 0) return s;
    if (mode == 2) triple_coef(cfg, is_pos, s, coef, l);
    if (coef == 0.f) return s;
    {
        Row<G, IT> d0 = g;
        dscore<G, IT>(d0, coef, cfg.l1, g);
    }
    // back through the two projections' normalisation: q = (g - (g.H) H) / |u|  (the clamp branch passes g / |u|)
    const float ch = ssh > 1e-12f ? dot<G, IT>(g, H) : 0.f, ct = sst > 1e-12f ? dot<G, IT>(g, T) : 0.f;
    Row<G, IT> qh, qt;
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        qh.v[it] = (g.v[it] - ch * H.v[it]) * ih;
        qt.v[it] = (ct * T.v[it] - g.v[it]) * itl;
    }
    const float bh = dot<G, IT>(qh, rp), bt = dot<G, IT>(qt, rp);
    Row<G, IT> o;
#pragma unroll
    for (int it = 0; it < IT; ++it) o.v[it] = qh.v[it] + bh * hp.v[it];
    atomic_row<G, IT>(ws.ent_grad + (int64_t)h * ld, ld, lane, o, 1.f);
#pragma unroll
    for (int it = 0; it < IT; ++it) o.v[it] = bh * yh.v[it];
    atomic_row<G, IT>(ws.ent_grad + (eb + h) * ld, ld, lane, o, 1.f);
#pragma unroll
    for (int it = 0; it < IT; ++it) o.v[it] = qt.v[it] + bt * tp.v[it];
    atomic_row<G, IT>(ws.ent_grad + (int64_t)t * ld, ld, lane, o, 1.f);
#pragma unroll
    for (int it = 0; it < IT; ++it) o.v[it] = bt * yt.v[it];
    atomic_row<G, IT>(ws.ent_grad + (eb + t) * ld, ld, lane, o, 1.f);
#pragma unroll
    for (int it = 0; it < IT; ++it) o.v[it] = ah * qh.v[it] + at * qt.v[it];
    atomic_row<G, IT>(ws.rel_copy(item % kRelCopies) + (rb + r) * ld, ld, lane, o, 1.f);
    atomic_row<G, IT>(ws.rel_copy(item % kRelCopies) + (int64_t)r * ld, ld, lane, g, 1.f);
    if (lane == 0) {
        ws.ent_touched[h] = 1.f; ws.ent_touched[t] = 1.f; ws.ent_touched[eb + h] = 1.f; ws.ent_touched[eb + t] = 1.f;
        ws.rel_touched[r] = 1.f; ws.rel_touched[rb + r] = 1.f;
    }
    return s;
}

template <int G, int IT>
__device__ float transh_triple(const float *__restrict__ ent, const float *__restrict__ rel, int ld, int lane,
                               int64_t item, int h, int r, int t, bool is_pos, const oea_step_cfg &cfg,
                               const StepWs &ws, int mode, float coef, float &l) {
    Row<G, IT> yh, yr, yt, yn, g;
    load_row<G, IT>(ent + (int64_t)h * ld, ld, lane, yh);
    load_row<G, IT>(rel + (int64_t)r * ld, ld, lane, yr);
    load_row<G, IT>(ent + (int64_t)t * ld, ld, lane, yt);
    load_normal<G, IT>(cfg.normal, r, ld, lane, yn);
    normalize<G, IT>(yh, cfg.ent_l2_norm);
    normalize<G, IT>(yr, cfg.rel_l2_norm);
    normalize<G, IT>(yt, cfg.ent_l2_norm);
    const float ah = dot<G, IT>(yh, yn), at = dot<G, IT>(yt, yn);
    float s = 0.f;
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const float d = (yh.v[it] - ah * yn.v[it]) + yr.v[it] - (yt.v[it] - at * yn.v[it]);
        g.v[it] = d;
        s += cfg.l1 ? fabsf(d) : d * d;
    }
    s = group_sum<G>(s);
    l = 0.f;
    if (mode == 0) return s;
    if (mode == 2) triple_coef(cfg, is_pos, s, coef, l);
    if (coef == 0.f) return s;
    {
        Row<G, IT> d0 = g;
        dscore<G, IT>(d0, coef, cfg.l1, g);
    }
    const float gdn = dot<G, IT>(g, yn);
    Row<G, IT> pg, gn;
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        pg.v[it] = g.v[it] - gdn * yn.v[it];
        gn.v[it] = (at - ah) * g.v[it] + gdn * (yt.v[it] - yh.v[it]);
    }
    atomic_row<G, IT>(ws.ent_grad + (int64_t)h * ld, ld, lane, pg, 1.f);
    atomic_row<G, IT>(ws.ent_grad + (int64_t)t * ld, ld, lane, pg, -1.f);
    atomic_row<G, IT>(ws.rel_copy(item % kRelCopies) + (int64_t)r * ld, ld, lane, g, 1.f);
    atomic_row<G, IT>(ws.nrm_copy(item % kRelCopies) + (int64_t)r * ld, ld, lane, gn, 1.f);
    if (lane == 0) { ws.ent_touched[h] = 1.f; ws.ent_touched[t] = 1.f; ws.rel_touched[r] = 1.f; ws.nrm_touched[r] = 1.f; }
    return s;
}

template <int G, int IT, int KIND>
__global__ __launch_bounds__(256) void triple_projected(
    const float *__restrict__ ent, const float *__restrict__ rel, int ld, const int32_t *__restrict__ pos,
    int64_t n_pos, const int32_t *__restrict__ neg, int64_t n_neg, oea_step_cfg cfg, StepWs ws) {
    const int lane = threadIdx.x % G;
    const int64_t grp = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int64_t ngrp = (int64_t)gridDim.x * blockDim.x / G;
    const bool margin = cfg.loss_kind == OEA_LOSS_MARGIN;
    const int64_t items = margin ? n_pos : n_pos + n_neg;
    double loss_local = 0.0;
    auto one = [&](int64_t item, const int32_t *tr, bool is_pos, int mode, float coef, float &l) {
        if (KIND == OEA_SCORE_TRANSD)
            return transd_triple<G, IT>(ent, rel, ld, lane, item, tr[0], tr[1], tr[2], is_pos, cfg, ws, mode, coef, l);
        return transh_triple<G, IT>(ent, rel, ld, lane, item, tr[0], tr[1], tr[2], is_pos, cfg, ws, mode, coef, l);
    };
    for (int64_t item = grp; item < items; item += ngrp) {
        float l;
        if (!margin) {
            const bool is_pos = item < n_pos;
            one(item, is_pos ? pos + 3 * item : neg + 3 * (item - n_pos), is_pos, 2, 0.f, l);
            if (lane == 0) loss_local += (double)l;
            continue;
        }
        // losses.py:15-27: sum relu(margin + s+ - s-), pos i paired with neg i; both are scored first, the active
        // pairs are evaluated again for their gradients (dL/ds+ = 1, dL/ds- = -1)
        float sc[2];
#pragma unroll 1
        for (int u = 0; u < 2; ++u) sc[u] = one(item, (u ? neg : pos) + 3 * item, u == 0, 0, 0.f, l);
        const float x = cfg.margin + sc[0] - sc[1];
        if (x <= 0.f) continue;
        if (lane == 0) loss_local += (double)x;
#pragma unroll 1
        for (int u = 0; u < 2; ++u) one(item, (u ? neg : pos) + 3 * item, u == 0, 1, u ? -1.f : 1.f, l);
    }
    block_loss_partial(loss_local, ws.partials);
}

// optimiser on the touched normal-vector rows: gradient back through BOTH normalisations
template <int G, int IT>
__global__ __launch_bounds__(256) void apply_normal_rows(int64_t n_rel, int ld, oea_step_cfg cfg, StepWs ws, int copies_folded) {
    const int lane = threadIdx.x % G;
    const int64_t grp = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int64_t ngrp = (int64_t)gridDim.x * blockDim.x / G;
    for (int64_t row = grp; row < n_rel; row += ngrp) {
        if (ws.nrm_touched[row] == 0) continue;
        float *v = cfg.normal + row * ld;
        Row<G, IT> rv, rg, y1, y2;
        grad_t q[IT];
        load_row<G, IT>(v, ld, lane, rv);
        load_grad_raw<G, IT>(ws.nrm_grad + row * ld, ld, lane, q);
        for (int cp = 1; cp < kRelCopies && !copies_folded; ++cp) {
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                const int c = it * G + lane;
                if (c < ld) {
                    const grad_t x = ws.nrm_copy(cp)[row * ld + c];
                    if (x != 0) { q[it] += x; ws.nrm_copy(cp)[row * ld + c] = 0; }
                }
            }
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) rg.v[it] = oea::grad_val(q[it]);
        const float ss1 = sumsq<G, IT>(rv);
        const float inv1 = rsqrtf(fmaxf(ss1, 1e-12f));
#pragma unroll
        for (int it = 0; it < IT; ++it) y1.v[it] = rv.v[it] * inv1;
        const float ss2 = sumsq<G, IT>(y1);
        const float inv2 = rsqrtf(fmaxf(ss2, 1e-12f));
#pragma unroll
        for (int it = 0; it < IT; ++it) y2.v[it] = y1.v[it] * inv2;
        const float d2 = dot<G, IT>(y2, rg);
#pragma unroll
        for (int it = 0; it < IT; ++it) rg.v[it] = (rg.v[it] - y2.v[it] * d2) * inv2;
        const float d1 = ss1 > 1e-12f ? dot<G, IT>(y1, rg) : 0.f;
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int c = it * G + lane;
            if (c < ld) {
                const float gv = (rg.v[it] - y1.v[it] * d1) * inv1;
                if (cfg.opt_kind == OEA_OPT_ADAGRAD) {
                    const float a = cfg.normal_acc[row * ld + c] + gv * gv;
                    cfg.normal_acc[row * ld + c] = a;
                    v[c] = rv.v[it] - cfg.lr * gv / sqrtf(a);
                } else {
                    v[c] = rv.v[it] - cfg.lr * gv;
                }
                ws.nrm_grad[row * ld + c] = 0;
            }
        }
        if (lane == 0) ws.nrm_touched[row] = 0;
    }
}

// ---- kernel 2: optimiser on touched rows (relation rows first, then entity rows) -------------------
// Row's interface on float4 fragments (the fp32 scratch; ld % 4 == 0: a float4 is inside the row or past it).  A group of G lanes
// holds IT4 = ceil(ld / (4 G)) float4 per row (ld = 100, G = 16: two loads per row instead of seven dwords), a quarter of the memory
// instructions per row stream: the planned optimiser is ONE residency of latency-bound chains (record -> rows -> stores), so what
// it issues per row is what it costs.  dot_partial adds ((x x + y y) + z z) + w w per fragment to the running sum and add_signed is
// an fma by +-1 (exact): this layout's order and form, which fix its bits.
template <int G, int IT4>
struct Row4 {
    static constexpr int kLanes = G, kFrags = IT4, kWidth = 4;
    float v[IT4][4];
    __device__ __forceinline__ static int col(int it, int lane) { return (it * G + lane) * 4; }
    __device__ __forceinline__ float s(int it, int j) const { return v[it][j]; }
    __device__ __forceinline__ static void put(float *p, const float (&x)[4]) { oea::st4(p, make_float4(x[0], x[1], x[2], x[3])); }
    __device__ __forceinline__ static void zero(float *p) { oea::st4(p, make_float4(0.f, 0.f, 0.f, 0.f)); }
    __device__ __forceinline__ void load(const float *__restrict__ base, int ld, int lane) {
#pragma unroll
        for (int it = 0; it < IT4; ++it) {
            const int c = col(it, lane);
            const float4 f = c < ld ? oea::ld4(base + c) : make_float4(0.f, 0.f, 0.f, 0.f);
            v[it][0] = f.x; v[it][1] = f.y; v[it][2] = f.z; v[it][3] = f.w;
        }
    }
    __device__ __forceinline__ void load_grad(const float *__restrict__ base, int ld, int lane) { load(base, ld, lane); }
    __device__ __forceinline__ float dot_partial(const Row4 &o) const {
        float p = 0.f;
#pragma unroll
        for (int it = 0; it < IT4; ++it) p += v[it][0] * o.v[it][0] + v[it][1] * o.v[it][1] + v[it][2] * o.v[it][2] + v[it][3] * o.v[it][3];
        return p;
    }
    __device__ __forceinline__ void set_signed(const Row4 &o, bool neg) {
        const float sg = neg ? -1.f : 1.f;
#pragma unroll
        for (int it = 0; it < IT4; ++it)
#pragma unroll
            for (int j = 0; j < 4; ++j) v[it][j] = sg * o.v[it][j];
    }
    __device__ __forceinline__ void add_signed(const Row4 &o, bool neg) {
        const float sg = neg ? -1.f : 1.f;
#pragma unroll
        for (int it = 0; it < IT4; ++it)
#pragma unroll
            for (int j = 0; j < 4; ++j) v[it][j] = fmaf(sg, o.v[it][j], v[it][j]);
    }
    __device__ __forceinline__ void add_and_clear(const Row4 &o, float *g, int ld, int lane) {
#pragma unroll
        for (int it = 0; it < IT4; ++it) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[it][j] += o.v[it][j];
            if (col(it, lane) < ld) zero(g + col(it, lane));
        }
    }
};

// one relation row: fetched together with its flag (most relations of a batch are touched); sums (fixed order) and clears the
// scratch copies
template <int G, int IT>
__device__ __forceinline__ void apply_relation_row(int64_t row, float *__restrict__ rel, float *__restrict__ rel_acc, int ld, int lane,
                                                   const oea_step_cfg &cfg, const StepWs &ws, int copies_folded) {
    float *v = rel + row * ld;
    float *acc = rel_acc + row * ld;
    grad_t *g = ws.rel_grad + row * ld;
    const float flag = (float)ws.rel_touched[row];
    Row<G, IT> rv, rg, ra;
    grad_t q[IT];                       // raw scratch elements: the copies are summed exactly in the fixed-point build
    load_row<G, IT>(v, ld, lane, rv);
    load_grad_raw<G, IT>(g, ld, lane, q);
    if (cfg.opt_kind == OEA_OPT_ADAGRAD) load_row<G, IT>(acc, ld, lane, ra);
    if (flag == 0.f) return;
    if (!copies_folded) {               // sum (fixed order) and clear the other copies
        // copies fetched together (all loads issued before use).  The fixed-point build keeps this loop rolled: unrolled, its
        // int64 elements (two registers each) took the kernel from 120 to 172 VGPRs = from 4 to 2 waves per SIMD, and the
        // latency-bound 15K shape paid double (11.3 -> 23.7 us, gpurun_out r04a)
        constexpr int CB = IT <= 4 ? 5 : 1;
#ifdef OEA_DET_SCRATCH
#pragma unroll 1
#endif
        for (int cp0 = 1; cp0 < kRelCopies; cp0 += CB) {
            grad_t tmp[CB][IT];
#pragma unroll
            for (int u = 0; u < CB; ++u)
#pragma unroll
                for (int it = 0; it < IT; ++it) {
                    const int c = it * G + lane;
                    tmp[u][it] = (cp0 + u < kRelCopies && c < ld) ? ws.rel_copy(cp0 + u)[row * ld + c] : (grad_t)0;
                }
#pragma unroll
            for (int u = 0; u < CB; ++u)
#pragma unroll
                for (int it = 0; it < IT; ++it) {
                    const int c = it * G + lane;
                    q[it] += tmp[u][it];
                    if (cp0 + u < kRelCopies && c < ld && tmp[u][it] != 0) ws.rel_copy(cp0 + u)[row * ld + c] = 0;
                }
        }
    }
#pragma unroll
    for (int it = 0; it < IT; ++it) rg.v[it] = oea::grad_val(q[it]);
    apply_one_row(v, acc, g, ws.rel_touched + row, ld, lane, cfg.rel_l2_norm, cfg, rv, rg, ra);
}

// The loss partials of the scoring kernel into *loss_accum by a whole block of 256 (add_loss_partials_wave of step_rows.h: by one
// wave): every lane a strided share (all loads in flight), then a fixed tree.  n_partials <= kMaxPlanPartials, laid out by
// plan_partial; the ones past kMaxBlocks are cleared once read (step_rows.h: that part of the workspace is zero between steps).
__device__ __forceinline__ void add_loss_partials_block(const StepWs &ws, int n_partials, double *__restrict__ loss_accum) {
    constexpr int kPerLane = 32, kLow = kMaxBlocks / 256;
    static_assert(kMaxPlanPartials <= kPerLane * 256 && kMaxBlocks % 256 == 0, "the block reads 32 partials per lane");
    __shared__ double sp[256];
    double v[kPerLane];
#pragma unroll
    for (int u = 0; u < kPerLane; ++u) { const int i = u * 256 + (int)threadIdx.x; v[u] = i < n_partials ? *plan_partial(ws, i) : 0.0; }
    double acc = 0.0;
#pragma unroll
    for (int u = 0; u < kPerLane; ++u) acc += v[u];
#pragma unroll
    for (int u = kLow; u < kPerLane; ++u) { const int i = u * 256 + (int)threadIdx.x; if (i < n_partials) *plan_partial(ws, i) = 0.0; }
    sp[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sp[threadIdx.x] += sp[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss_accum += sp[0];
}

// Work item w of the grid: w < n_rel -> relation row w (sums its 16 scratch copies); else R consecutive entity rows.
// The kernel is a few thousand very short waves (three row loads, two reductions, two row stores): R > 1 keeps R rows'
// loads in flight per group and divides the wave count by R (latency-bound at the 15K shape).
template <int G, int IT, int R>
__global__ __launch_bounds__(256) void apply_rows(float *__restrict__ ent, float *__restrict__ ent_acc,
                                                  int64_t n_ent, float *__restrict__ rel,
                                                  float *__restrict__ rel_acc, int64_t n_rel, int ld,
                                                  oea_step_cfg cfg, StepWs ws, int n_partials,
                                                  double *__restrict__ loss_accum, int copies_folded, int flag_first) {
    const int lane = threadIdx.x % G;
    const int64_t grp = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int64_t ngrp = (int64_t)gridDim.x * blockDim.x / G;
    const int64_t n_items = n_rel + (n_ent + R - 1) / R;
    for (int64_t w = grp; w < n_items; w += ngrp) {
        if (w >= n_rel) {                                // ---- R entity rows ---------------------------------------
            const int64_t row0 = (w - n_rel) * R;
            float flag[R];
            Row<G, IT> rv[R], rg[R], ra[R];
            if (flag_first) {          // large tables: a batch leaves many rows untouched -- look before fetching 3 rows
                bool any = false;
#pragma unroll
                for (int r = 0; r < R; ++r) any |= row0 + r < n_ent && ws.ent_touched[row0 + r] != 0;
                if (!any) continue;
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int64_t row = row0 + r < n_ent ? row0 + r : n_ent - 1;
                flag[r] = row0 + r < n_ent ? (float)ws.ent_touched[row] : 0.f;
                load_row<G, IT>(ent + row * ld, ld, lane, rv[r]);
                load_grad_row<G, IT>(ws.ent_grad + row * ld, ld, lane, rg[r]);
                if (cfg.opt_kind == OEA_OPT_ADAGRAD) load_row<G, IT>(ent_acc + row * ld, ld, lane, ra[r]);
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (flag[r] == 0.f) continue;
                const int64_t row = row0 + r;
                apply_one_row(ent + row * ld, ent_acc + row * ld, ws.ent_grad + row * ld, ws.ent_touched + row, ld,
                                     lane, cfg.ent_l2_norm, cfg, rv[r], rg[r], ra[r]);
            }
            continue;
        }
        apply_relation_row<G, IT>(w, rel, rel_acc, ld, lane, cfg, ws, copies_folded);
    }
    if (blockIdx.x == 0 && threadIdx.x < 64) add_loss_partials_wave(ws, n_partials, loss_accum);
}

// ---- kernel 2', round 6: the optimiser of a PLANNED step (step_plan.h), one launch, four kinds of blocks ----------------------------------
//   [0, rel_blocks)        relation rows, one lane group per row as in apply_rows (16 scratch copies summed in order);
//   (plan blocks, listed third in the grid)    one lane group per DISTINCT entity row the step's positives refer to as head or tail and that is no hub:
//                          gradient = the sum of its plan entries (sign, slot) over contrib[slot] in the plan's order -- the batch
//                          order, whatever the hardware does -- plus the row of the atomic scratch where its touched flag is up (an
//                          active negative corrupted INTO this row).  Chain of dependent loads: step_first -> record -> rows;
//   [.., + scan_blocks)    what the plan does not list: entity rows whose touched flag is up (corrupted rows of active negatives, hub
//                          rows, rows of positives outside the rule: a few thousand of 200,000).  A wave reads 64 flags with one
//                          load and its groups take the flagged rows of the ballot; chunk c = rows {c, c + n_chunk, ...}: entity ids
//                          are degree-ordered (read.py:64-79), 64 CONSECUTIVE rows at the head of the table are all hubs and one
//                          wave would work through them alone.  Rows the plan sums are left to their group (membership map);
//   last block             the loss partials, 256 lanes + a fixed tree (one wave walking 2,500 partials took 18 us).
// Same update everywhere: gradient back through the normalisation, Adagrad / SGD (apply_one_row).
// V4: the entity rows (plan rows and flag-scan rows) travel as float4 (Row4) instead of dwords (Row); relation rows are dwords either way.
template <int G, int IT, bool V4>
__global__ __launch_bounds__(256) void apply_step_plan(float *__restrict__ ent, float *__restrict__ ent_acc, int64_t n_ent,
                                                       float *__restrict__ rel, float *__restrict__ rel_acc, int64_t n_rel, int ld,
                                                       oea_step_cfg cfg, StepWs ws, int n_partials, double *__restrict__ loss_accum,
                                                       int copies_folded, int rel_blocks, int scan_blocks,
                                                       const uint4 *__restrict__ recs, const uint32_t *__restrict__ vals,
                                                       const int32_t *__restrict__ step_first, int s, const uint8_t *__restrict__ inplan,
                                                       const float *__restrict__ contrib) {
    using F = std::conditional_t<V4, Row4<G, (IT + 3) / 4>, Row<G, IT>>;
    constexpr int GPB = 256 / G, GPW = 64 / G;
    const int lane = threadIdx.x % G;
    const int b = (int)blockIdx.x, nb = (int)gridDim.x;
    if (b < rel_blocks) {
        for (int64_t row = (int64_t)b * GPB + threadIdx.x / G; row < n_rel; row += (int64_t)rel_blocks * GPB)
            apply_relation_row<G, IT>(row, rel, rel_acc, ld, lane, cfg, ws, copies_folded);
    } else if (b >= rel_blocks + scan_blocks && b < nb - 1) {
        const int plan_blocks = nb - 1 - rel_blocks - scan_blocks;
        const int64_t grp = (int64_t)(b - rel_blocks - scan_blocks) * GPB + threadIdx.x / G, ngrp = (int64_t)plan_blocks * GPB;
        const int64_t i1 = step_first[s + 1];
        for (int64_t i = step_first[s] + grp; i < i1; i += ngrp) {
            const uint4 rec = recs[i];                                 // {row, first entry, entries, first entry's value}
            if (rec.z > oea::kPlanHubEntries) continue;                // a hub of this step: its gradient went through the atomic scratch
            const int64_t row = rec.x;
            const uint32_t e0 = rec.y, e1 = rec.y + rec.z, v0 = rec.w;
            const float flag = (float)ws.ent_touched[row];
            F rv, ra, rg, rc;
            rv.load(ent + row * ld, ld, lane);
            if (cfg.opt_kind == OEA_OPT_ADAGRAD) ra.load(ent_acc + row * ld, ld, lane);
            rc.load(contrib + (int64_t)(v0 & 0x7fffffffu) * ld, ld, lane);
            rg.set_signed(rc, v0 >> 31);
            for (uint32_t e = e0 + 1; e < e1; e += 3) {                // further references to the row, in batch order, three in flight
                uint32_t ve[3];
                F r3[3];
#pragma unroll
                for (int u = 0; u < 3; ++u) ve[u] = vals[min(e + u, e1 - 1)];
#pragma unroll
                for (int u = 0; u < 3; ++u) r3[u].load(contrib + (int64_t)(ve[u] & 0x7fffffffu) * ld, ld, lane);
#pragma unroll
                for (int u = 0; u < 3; ++u)
                    if (e + u < e1) rg.add_signed(r3[u], ve[u] >> 31);
            }
            if (flag != 0.f) {                                         // + what the atomic scratch holds for this row
                grad_t *g = ws.ent_grad + row * ld;
                F rs;
                rs.load_grad(g, ld, lane);
                rg.add_and_clear(rs, g, ld, lane);
                if (lane == 0) ws.ent_touched[row] = 0;
            }
            apply_one_row<false>(ent + row * ld, ent_acc + row * ld, nullptr, nullptr, ld, lane, cfg.ent_l2_norm, cfg, rv, rg, ra);
        }
    } else if (b < nb - 1) {
        // (the scan's blocks come BEFORE the plan's in the grid: its waves work through their flagged rows one group-load at a time --
        //  the long pole late in training, when many negatives are active -- and should not wait for the plan's blocks to retire)
        const int first = rel_blocks;
        const int wl = threadIdx.x & 63, gw = wl / G;
        const int64_t wave = (int64_t)(b - first) * 4 + (threadIdx.x >> 6), nwave = (int64_t)scan_blocks * 4;
        const int64_t n_chunk = (n_ent + 63) / 64;
        const uint8_t *mine = inplan + (int64_t)s * n_ent;
        for (int64_t chunk = wave; chunk < n_chunk; chunk += nwave) {
            const int64_t r = (int64_t)wl * n_chunk + chunk;
            const bool todo = r < n_ent && (float)ws.ent_touched[r] != 0.f && mine[r] == 0;
            unsigned long long mask = __ballot(todo);
            while (mask) {
                int64_t row = -1;
#pragma unroll
                for (int q = 0; q < GPW; ++q)
                    if (mask) {
                        const int bit = __builtin_ctzll(mask);
                        mask &= mask - 1;
                        if (gw == q) row = (int64_t)bit * n_chunk + chunk;
                    }
                if (row >= 0) {
                    F rv, rg, ra;
                    rv.load(ent + row * ld, ld, lane);
                    rg.load_grad(ws.ent_grad + row * ld, ld, lane);
                    if (cfg.opt_kind == OEA_OPT_ADAGRAD) ra.load(ent_acc + row * ld, ld, lane);
                    apply_one_row(ent + row * ld, ent_acc + row * ld, ws.ent_grad + row * ld, ws.ent_touched + row, ld, lane,
                                  cfg.ent_l2_norm, cfg, rv, rg, ra);
                }
            }
        }
    } else {
        add_loss_partials_block(ws, n_partials, loss_accum);
    }
}

// ---- kernel 2b: optimisers whose update is DENSE (tf.train.AdamOptimizer / AdadeltaOptimizer, optimizers.py:13-16) -------
// The tables are l2_normalize(variable): the gradient of a gather comes back through the normalisation as a dense
// tensor, so TF's dense kernels run -- Adam moves every row every step (m and v decay where the gradient is zero),
// Adadelta's accumulators decay everywhere.  state: [2, rows, ld] = (m, v) for Adam, (accum, accum_update) for
// Adadelta.  The relation scratch copies must have been folded into copy 0 (fold_rel_copies_kernel).
template <int G, int IT>
__global__ __launch_bounds__(256) void apply_rows_dense(float *__restrict__ ent, float *__restrict__ ent_state,
                                                        int64_t n_ent, float *__restrict__ rel,
                                                        float *__restrict__ rel_state, int64_t n_rel, int ld,
                                                        oea_step_cfg cfg, StepWs ws, int n_partials,
                                                        double *__restrict__ loss_accum, float lr_t) {
    const int lane = threadIdx.x % G;
    const int64_t grp = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int64_t ngrp = (int64_t)gridDim.x * blockDim.x / G;
    for (int64_t row_all = grp; row_all < n_ent + n_rel; row_all += ngrp) {
        const bool is_rel = row_all < n_rel;
        const int64_t row = is_rel ? row_all : row_all - n_rel;
        const int64_t rows = is_rel ? n_rel : n_ent;
        flag_t *touched = is_rel ? ws.rel_touched : ws.ent_touched;
        float *v = (is_rel ? rel : ent) + row * ld;
        float *s0 = (is_rel ? rel_state : ent_state) + row * ld;
        float *s1 = s0 + rows * (int64_t)ld;
        grad_t *g = (is_rel ? ws.rel_grad : ws.ent_grad) + row * ld;
        const int on = is_rel ? cfg.rel_l2_norm : cfg.ent_l2_norm;
        const float flag = (float)touched[row];
        // Adadelta WITHOUT the l2_normalize in front of the lookup: TF's gradient is IndexedSlices and SparseApplyAdadelta
        // only visits the gathered rows -- the accumulators of untouched rows do not decay.  (With the normalisation the
        // gradient is dense; TF1's sparse Adam decays every row either way: optimizer._apply_sparse_shared.)
        if (cfg.opt_kind == OEA_OPT_ADADELTA && !on && flag == 0.f) continue;
        Row<G, IT> rv, rg, r0, r1;
        load_row<G, IT>(v, ld, lane, rv);
        load_grad_row<G, IT>(g, ld, lane, rg);
        load_row<G, IT>(s0, ld, lane, r0);
        load_row<G, IT>(s1, ld, lane, r1);
        float inv = 1.f, ydg = 0.f;
        if (on) {
            const float ss = sumsq<G, IT>(rv);
            inv = rsqrtf(fmaxf(ss, 1e-12f));
            float dot = 0.f;
#pragma unroll
            for (int it = 0; it < IT; ++it) dot += rv.v[it] * rg.v[it];
            dot = group_sum<G>(dot) * inv;
            ydg = ss > 1e-12f ? dot : 0.f;
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int c = it * G + lane;
            if (c < ld) {
                const float gv = on ? (rg.v[it] - rv.v[it] * inv * ydg) * inv : rg.v[it];
                if (cfg.opt_kind == OEA_OPT_ADAM) {          // training_ops ApplyAdam
                    const float m = r0.v[it] + (gv - r0.v[it]) * (1.f - cfg.beta1);
                    const float vv = r1.v[it] + (gv * gv - r1.v[it]) * (1.f - cfg.beta2);
                    s0[c] = m; s1[c] = vv;
                    v[c] = rv.v[it] - lr_t * m / (sqrtf(vv) + cfg.eps);
                } else {                                     // ApplyAdadelta (rho = beta1)
                    const float acc = r0.v[it] * cfg.beta1 + gv * gv * (1.f - cfg.beta1);
                    const float upd = sqrtf(r1.v[it] + cfg.eps) * rsqrtf(acc + cfg.eps) * gv;
                    s0[c] = acc;
                    s1[c] = r1.v[it] * cfg.beta1 + upd * upd * (1.f - cfg.beta1);
                    v[c] = rv.v[it] - cfg.lr * upd;
                }
                if (flag != 0.f) g[c] = 0;
            }
        }
        if (flag != 0.f && lane == 0) touched[row] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x < 64) add_loss_partials_wave(ws, n_partials, loss_accum);
}

// data parallel: fold relation copies 1.. into copy 0 (and clear them) so that only copy 0 is exchanged
__global__ void fold_rel_copies_kernel(StepWs ws, int64_t n, int with_normal) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        grad_t sum = 0;
#pragma unroll
        for (int c = 0; c < kRelCopies - 1; ++c) {
            const grad_t v = ws.rel_extra[c * ws.rel_copy_stride + i];
            if (v != 0) { sum += v; ws.rel_extra[c * ws.rel_copy_stride + i] = 0; }
        }
        if (sum != 0) ws.rel_grad[i] += sum;
        if (with_normal) {
            grad_t sn = 0;
#pragma unroll
            for (int c = 0; c < kRelCopies - 1; ++c) {
                const grad_t v = ws.nrm_extra[c * ws.rel_copy_stride + i];
                if (v != 0) { sn += v; ws.nrm_extra[c * ws.rel_copy_stride + i] = 0; }
            }
            if (sn != 0) ws.nrm_grad[i] += sn;
        }
    }
}

// grad[ids[i], c] += src[i, c]  (gradients w.r.t. NORMALISED rows produced outside the fused step,
// e.g. MTransE's mapping loss, approaches/mtranse.py:84-96) + touched flags, so that apply_rows
// pulls them through the normalisation and the optimiser like any other row gradient.
__global__ void scatter_rows_kernel(grad_t *__restrict__ grad, flag_t *__restrict__ touched, int ld,
                                    const int32_t *__restrict__ ids, int64_t n, const float *__restrict__ src,
                                    int src_ld) {
    const int64_t total = n * ld;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / ld;
        const int c = (int)(i - row * ld);
        const float v = src[row * src_ld + c];
        const int32_t id = ids[row];
        if (v != 0.f) oea::grad_add(grad + (int64_t)id * ld + c, v);
        if (c == 0) touched[id] = 1;
    }
}

// triple_grouped specialised on (loss kind, norm) -- the per-triple losses that reach it (margin pairs go to
// triple_generic); OEA_STEP_RUNTIME_KIND=1 keeps the one kernel with the run-time switch (experiments).
// OEA_STEP_WAVE = 0: triple_grouped (two positives per wave) everywhere
static bool step_wave_enabled() {
    static const int env = [] { const char *e = getenv("OEA_STEP_WAVE"); return e ? atoi(e) : 1; }();
    return env != 0;
}

// triple_wave's launch: waves per workgroup and workgroups, decided by wave_geometry (below, next to wave_rule) and nowhere else
struct WaveGeometry { int waves, grid; };

template <int IT64>
void launch_wave(const WaveGeometry &g, hipStream_t st, const float *ent, const float *rel, int ld, const int32_t *pos,
                 int64_t n_pos, const int32_t *neg, const oea_step_cfg &cfg, const StepWs &ws, float *contrib = nullptr,
                 const uint32_t *pflags = nullptr, const uint32_t *order = nullptr) {
    const int k = cfg.neg_group_k;
    static const int dbg = [] { const char *e = getenv("OEA_STEP_WAVE_DBG"); return e ? atoi(e) : 0; }();
#define OEA_WAVE(L1, KT)                                                                                                               \
    do {                                                                                                                               \
        if constexpr (!oea::kDetScratch) {  /* PLAN = true: where a plan can exist (kPlanInstance) */                                  \
            if (contrib) {  /* WPB = g.waves: 8 exists at ld <= 128 alone (wave_geometry gives ld > 128 four waves) */                  \
                if constexpr (IT64 <= 2) {                                                                                             \
                    if (g.waves == 8) {                                                                                                \
                        oea::launch_timed(triple_wave<IT64, L1, KT, true, 8>, g.grid, 8 * 64, st, ent, rel, ld, pos, n_pos, neg, k, cfg, ws, dbg, contrib, pflags, order);   \
                        break;                                                                                                         \
                    }                                                                                                                  \
                }                                                                                                                      \
                oea::launch_timed(triple_wave<IT64, L1, KT, true, 4>, g.grid, 4 * 64, st, ent, rel, ld, pos, n_pos, neg, k, cfg, ws, dbg, contrib, pflags, order);   \
                break;                                                                                                                 \
            }                                                                                                                          \
        }                                                                                                                              \
        oea::launch_timed(triple_wave<IT64, L1, KT, false>, g.grid, g.waves * 64, st, ent, rel, ld, pos, n_pos, neg, k, cfg, ws, dbg, contrib, pflags, nullptr);   \
    } while (0)
    if (k == 10) { if (cfg.l1) OEA_WAVE(1, 10); else OEA_WAVE(0, 10); }
    else { if (cfg.l1) OEA_WAVE(1, 0); else OEA_WAVE(0, 0); }
#undef OEA_WAVE
}

// OEA_STEP_RUNTIME_KIND=1 (experiments): triple_grouped with the run-time switch of loss kind and norm, everywhere
static bool step_runtime_kind() {
    static const int env = [] { const char *e = getenv("OEA_STEP_RUNTIME_KIND"); return e ? atoi(e) : 0; }();
    return env != 0;
}

// THE rule of triple_wave, and with it of the epoch plan: only triple_wave stores a positive's rows into the plan's contrib and
// honours its pflags, so launch_grouped (wave or grouped kernel) and oea_step_plan_supported (plan or no plan) both ask here and
// nowhere else.  One wave per positive: the per-triple "limited" loss on normalised rows, 1..10 grouped negatives, rows of at most
// 256 columns, tables whose byte offsets fit the instruction's 32-bit scalar offset.
static bool wave_rule(const oea_step_cfg &cfg, int64_t n_ent, int64_t n_rel, int32_t ld) {
    return cfg.score_kind == OEA_SCORE_TRANSE && cfg.loss_kind == OEA_LOSS_LIMITED && cfg.ent_l2_norm && cfg.rel_l2_norm &&
           cfg.neg_group_k >= 1 && cfg.neg_group_k <= 10 && ld <= 256 &&
           std::max(n_ent, n_rel) * (int64_t)ld * (int64_t)sizeof(grad_t) < ((int64_t)1 << 30) && step_wave_enabled() &&
           !step_runtime_kind();
}

// THE launch geometry of triple_wave, for launch_grouped's launch and for launch_step's count of the loss partials (one per
// workgroup).  ld > 128: 4 waves, one workgroup per 4 positives.  ld <= 128 without a plan: 8 waves, one per 8 positives -- both
// are loss_partials' count, the grid triple_grouped would take.  ld <= 128 with a plan: 4 waves, one workgroup per 4 positives, up to
// kMaxPlanPartials of them (the grid-stride loop takes the rest): a 4-wave workgroup fits the slots that the side stream's
// 256-thread workgroups (the epoch sampler's 49,600) leave one at a time, where an 8-wave workgroup needs two slots on every SIMD of
// one CU at the same moment and waits for the sampler to end.  OEA_STEP_WAVE_BLOCK (A/B runs, ld <= 128, plan or
// not): 512 = 8 waves per 8 positives, the geometry before this rule; 256 = 4 waves per 8 positives, two slots per wave.
static WaveGeometry wave_geometry(int32_t ld, int64_t n_pos, bool planned) {
    static const int blk_env = [] { const char *e = getenv("OEA_STEP_WAVE_BLOCK"); return e ? atoi(e) : 0; }();
    const int per8 = std::max(loss_partials(ld, n_pos), 1);      // (per 4 at ld > 128)
    if (ld > 128) return {4, per8};
    if (blk_env == 256 || blk_env == 512) return {blk_env / 64, per8};
    if (!planned) return {8, per8};
    return {4, (int)std::min<int64_t>(std::max<int64_t>(oea::ceil_div(n_pos, 4), 1), kMaxPlanPartials)};
}

// The instances of for_row_width's ladder that wave_rule can send to triple_wave (ld <= 256), and with them the plan's: the kernels
// of a planned step are built for these alone, and in the fp32 build alone (oea_step_plan_supported refuses the fixed-point build)
template <int G, int IT>
constexpr bool kWaveInstance = (G == 32 && IT <= 4) || (G == 64 && IT == 4);
template <int G, int IT>
constexpr bool kPlanInstance = kWaveInstance<G, IT> && !oea::kDetScratch;

// nb, block: triple_grouped's launch; where wave_rule sends the step to triple_wave, wave_geometry alone decides
template <int G, int IT>
void launch_grouped(int nb, int block, hipStream_t st, const float *ent, const float *rel, int ld, const int32_t *pos,
                    int64_t n_pos, const int32_t *neg, const oea_step_cfg &cfg, const StepWs &ws, bool wave, float *contrib = nullptr,
                    const uint32_t *pflags = nullptr, const uint32_t *order = nullptr) {
    const bool runtime_kind = step_runtime_kind();
    const int k = cfg.neg_group_k;
    // one wave per positive (round 6) where wave_rule says so (wave = its answer; ld <= 256 are exactly the instances below), in
    // wave_geometry's workgroups: launch_step counts the loss partials by the same rule (a planned step: contrib != nullptr)
    if constexpr (kWaveInstance<G, IT>) {
        if (wave) {
            constexpr int IT64 = G == 32 ? (IT + 1) / 2 : 4;
            const WaveGeometry g = wave_geometry(ld, n_pos, contrib != nullptr);
            launch_wave<IT64>(g, st, ent, rel, ld, pos, n_pos, neg, cfg, ws, contrib, pflags, order);
            return;
        }
    }
#define OEA_GROUPED(LOSS, L1) oea::launch_timed(triple_grouped<G, IT, LOSS, L1>, nb, block, st, ent, rel, ld, pos, n_pos, neg, k, cfg, ws)
    if (runtime_kind) OEA_GROUPED(-1, -1);
    else if (cfg.loss_kind == OEA_LOSS_LIMITED) { if (cfg.l1) OEA_GROUPED(OEA_LOSS_LIMITED, 1); else OEA_GROUPED(OEA_LOSS_LIMITED, 0); }
    else if (cfg.loss_kind == OEA_LOSS_LOGISTIC) { if (cfg.l1) OEA_GROUPED(OEA_LOSS_LOGISTIC, 1); else OEA_GROUPED(OEA_LOSS_LOGISTIC, 0); }
    else if (cfg.loss_kind == OEA_LOSS_POSITIVE) { if (cfg.l1) OEA_GROUPED(OEA_LOSS_POSITIVE, 1); else OEA_GROUPED(OEA_LOSS_POSITIVE, 0); }
    else OEA_GROUPED(-1, -1);
#undef OEA_GROUPED
}

template <int G, int IT>
int launch_step(float *ent, float *ent_acc, int64_t n_ent, float *rel, float *rel_acc, int64_t n_rel,
                int32_t ld, const int32_t *pos, int64_t n_pos, const int32_t *neg, int64_t n_neg,
                const oea_step_cfg &cfg, const StepWs &ws, double *loss_accum, int phase, hipStream_t st,
                const oea::StepPlanView *plan = nullptr, int plan_step = 0, int64_t plan_first_pos = 0) {
    const int block = 256, gpb = block / G;
    const bool transh = cfg.score_kind == OEA_SCORE_TRANSH, transd = cfg.score_kind == OEA_SCORE_TRANSD;
    const bool dense_opt = cfg.opt_kind == OEA_OPT_ADAM || cfg.opt_kind == OEA_OPT_ADADELTA;
    // TransH with a per-triple loss on the sampler's grouped layout keeps its grouped kernel; margin pairs, free
    // negative lists and TransD take the one-item-per-group kernel
    const bool transh_grouped = transh && cfg.loss_kind != OEA_LOSS_MARGIN && (n_neg == 0 || cfg.neg_group_k > 0);
    const bool projected = transd || (transh && !transh_grouped);
    const bool grouped = transh_grouped || (!projected && cfg.neg_group_k > 0 && cfg.loss_kind != OEA_LOSS_MARGIN);
    const int64_t items = step_items(cfg, n_pos, n_neg);
    // (G is for_row_width's: 32 up to ld 128, 64 beyond.)  A planned step is triple_wave's (oea_step_plan_supported asks wave_rule):
    // one partial per workgroup of wave_geometry, up to kMaxPlanPartials and laid out by plan_partial (step_rows.h).  Only
    // apply_step_plan's add_loss_partials_block reads that layout (and clears the partials past kMaxBlocks); add_loss_partials_wave
    // of every other optimiser kernel reads ws.partials[0 .. n_part) -- so a planned step must end in apply_step_plan, which
    // the SGD / Adagrad branch below does for every plan and which oea_step_plan_supported promises (no dense optimiser).
    const bool planned_wave = plan && items > 0 && wave_rule(cfg, n_ent, n_rel, ld);
    if (planned_wave && dense_opt) {
        oea::set_error("a plan with a dense optimiser (opt_kind %d): its loss partials have no reader", (int)cfg.opt_kind);
        return OEA_EUNSUPPORTED;
    }
    const int n_part = planned_wave ? wave_geometry(ld, n_pos, true).grid : loss_partials(ld, items);
    const int nb1 = std::max(loss_partials(ld, items), 1);     // triple_grouped's and the other kernels' grid (launch_grouped's nb)
    // profiling events, 4 per STEP: [m0 fwd_bwd m1] ... [m2 apply m3], each pair attached to its kernel's dispatch
    // (oea::launch_timed); a GRAD call takes the first pair and decides whether the step is sampled, the APPLY call
    // that follows takes the second pair
    if (phase != OEA_PHASE_APPLY) {
        oea::prof_call();
        if (transd)
            oea::launch_timed(triple_projected<G, IT, OEA_SCORE_TRANSD>, nb1, block, st, ent, rel, ld, pos, n_pos, neg, n_neg, cfg, ws);
        else if (projected)
            oea::launch_timed(triple_projected<G, IT, OEA_SCORE_TRANSH>, nb1, block, st, ent, rel, ld, pos, n_pos, neg, n_neg, cfg, ws);
        else if (transh)
            oea::launch_timed(triple_transh_grouped<G, IT>, nb1, block, st, ent, rel, ld, pos, n_pos, neg, n_neg ? cfg.neg_group_k : 0, cfg, ws);
        else if (grouped) {
            // OEA_STEP_REL_ORDER=0 (A/B runs): a planned step's waves take the positives in batch order and every wave issues its own
            // relation row, as before the plan carried rel_order
            static const bool rel_order_on = [] { const char *e = getenv("OEA_STEP_REL_ORDER"); return !(e && e[0] == '0'); }();
            // (plan->contrib != nullptr selects PLAN = true and the planned geometry there; with wave_rule it is planned_wave above
            // -- a plan always carries contrib, and an empty batch launches one idle workgroup either way)
            launch_grouped<G, IT>(nb1, block, st, ent, rel, ld, pos, n_pos, neg, cfg, ws, wave_rule(cfg, n_ent, n_rel, ld),
                                  plan ? plan->contrib : nullptr, plan ? plan->pflags + plan_first_pos : nullptr,
                                  plan && rel_order_on ? plan->rel_order + plan_first_pos : nullptr);
        }
        else
            oea::launch_timed(triple_generic<G, IT>, nb1, block, st, ent, rel, ld, pos, n_pos, neg, n_neg, cfg, ws);
        if (phase == OEA_PHASE_GRAD || dense_opt)
            fold_rel_copies_kernel<<<(unsigned)std::min<int64_t>(oea::ceil_div(n_rel * (int64_t)ld, 256), 1024), 256, 0, st>>>(
                ws, n_rel * (int64_t)ld, transh ? 1 : 0);
    }
    const int nb2 = (int)std::min<int64_t>(std::max<int64_t>(oea::ceil_div(n_ent + n_rel, gpb), 1), 16384);
    if (phase != OEA_PHASE_GRAD) {
        // the APPLY phase's event pair: start on its first launch, stop on its last (the plan path has two)
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        (void)oea::prof_pair(&ev0, &ev1);
        if (dense_opt) {
            // lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t)   (AdamOptimizer._apply_dense)
            const double t = (double)cfg.opt_t;
            const float lr_t = cfg.opt_kind == OEA_OPT_ADAM
                                   ? (float)((double)cfg.lr * std::sqrt(1.0 - std::pow((double)cfg.beta2, t)) / (1.0 - std::pow((double)cfg.beta1, t)))
                                   : cfg.lr;
            oea::launch_events(apply_rows_dense<G, IT>, nb2, block, st, ev0, ev1, ent, ent_acc, n_ent, rel, rel_acc, n_rel, ld, cfg, ws,
                              n_part, loss_accum, lr_t);
        } else {
            // rows per lane group: 1.  Measured at the 15K shape (gpurun_out r02a, in-epoch HIP events): R = 1 17.4 us,
            // R = 2 20.1, R = 4 20.4 -- more (shorter) waves hide the row latency better than more loads per wave.
            // OEA_APPLY_ROWS overrides (1 / 2 / 4) for experiments.
            static const int env_r = [] { const char *e = getenv("OEA_APPLY_ROWS"); return e ? atoi(e) : 0; }();
            const int R = env_r ? env_r : 1;
            const int folded = phase == OEA_PHASE_APPLY;
            // OEA_APPLY_FLAG_FIRST=1: look at the touched flag before fetching the three rows.  Measured (gpurun_out r02d):
            // 15K shape 11.1 -> 12.8 us, 100K shape 64.0 -> 72.5 us -- a batch touches most of the table at both shapes
            // and the dependent round trip costs more than the rows it saves; off by default.
            static const int flag_first_env = [] { const char *e = getenv("OEA_APPLY_FLAG_FIRST"); return e ? atoi(e) : 0; }();
            const int flag_first = plan ? 1 : flag_first_env;     // behind the plan pass few entity rows are left: look at the flag first
            auto nb = [&](int r) { return (int)std::min<int64_t>(std::max<int64_t>(oea::ceil_div(n_rel + oea::ceil_div(n_ent, r), gpb), 1), 16384); };
            // 16-lane groups (4 rows per wave, ceil(ld / 16) fragments per lane) when the tables do not fit the caches: the
            // kernel is then bound by HBM and the narrower groups waste fewer lanes on the row's tail -- 100K shape 64.5 ->
            // 54.9 us (step 0.139 -> 0.125 ms); at the 15K shape (latency-bound, cache-resident) they LOSE, 11.0 -> 16.3 us
            // (gpurun_out r02p).  OEA_APPLY_G16 = 0 / 1 overrides the size rule.
            const bool g16 = oea::apply_g16(n_ent, n_rel, ld);
            if (plan) {
                if constexpr (kPlanInstance<G, IT>) {
                    // ONE launch: relation rows | the plan's rows (gathered sums) | flagged rows the plan does not list | loss partials
                    const int64_t bound = 2 * n_pos;                       // at most two distinct rows per positive
                    const int pgpb = g16 && G == 32 ? 16 : gpb;
                    const int relb = (int)std::max<int64_t>(oea::ceil_div(n_rel, pgpb), 1);
                    const int planb = (int)std::min<int64_t>(std::max<int64_t>(oea::ceil_div(bound, pgpb), 1), 8192);
                    const int scanb = (int)std::min<int64_t>(std::max<int64_t>(oea::ceil_div(n_ent, 256), 1), 4096);
                    auto launch = [&](auto kernel) {
                        oea::launch_events(kernel, relb + planb + scanb + 1, block, st, ev0, ev1, ent, ent_acc, n_ent, rel, rel_acc, n_rel, ld, cfg,
                                           ws, n_part, loss_accum, folded, relb, scanb, plan->recs, plan->vals_b, plan->step_first, plan_step,
                                           plan->inplan, plan->contrib);
                    };
                    if (g16 && G == 32)
                        for_width16(ld, [&](auto it) {
                            constexpr int IT16 = decltype(it)::value;
                            // rows as float4; OEA_APPLY_V4=0: dword fragments
                            static const bool v4 = [] { const char *e = getenv("OEA_APPLY_V4"); return !(e && e[0] == '0'); }();
                            if (v4) launch(apply_step_plan<16, IT16, true>);
                            else launch(apply_step_plan<16, IT16, false>);
                        });
                    else
                        launch(apply_step_plan<G, IT, false>);
                } else {
                    oea::set_error("a plan for a row width no planned kernel is built for (ld %d)", ld);
                    return OEA_EUNSUPPORTED;
                }
            } else
            if (g16 && G == 32 && R == 1) {
                const int nbg = (int)std::min<int64_t>(std::max<int64_t>(oea::ceil_div(n_rel + n_ent, 16), 1), 16384);
                for_width16(ld, [&](auto it) {
                    oea::launch_events(apply_rows<16, decltype(it)::value, 1>, nbg, block, st, ev0, ev1, ent, ent_acc, n_ent, rel, rel_acc, n_rel,
                                       ld, cfg, ws, n_part, loss_accum, folded, flag_first);
                });
            } else
            if (R >= 4 && IT <= 4)
                oea::launch_events(apply_rows<G, IT, 4>, nb(4), block, st, ev0, ev1, ent, ent_acc, n_ent, rel, rel_acc, n_rel, ld, cfg, ws, n_part, loss_accum, folded, flag_first);
            else if (R >= 2 && IT <= 8)
                oea::launch_events(apply_rows<G, IT, 2>, nb(2), block, st, ev0, ev1, ent, ent_acc, n_ent, rel, rel_acc, n_rel, ld, cfg, ws, n_part, loss_accum, folded, flag_first);
            else
                oea::launch_events(apply_rows<G, IT, 1>, nb(1), block, st, ev0, ev1, ent, ent_acc, n_ent, rel, rel_acc, n_rel, ld, cfg, ws, n_part, loss_accum, folded, flag_first);
        }
        if (transh)
            apply_normal_rows<G, IT><<<(unsigned)std::max<int64_t>(oea::ceil_div(n_rel, gpb), 1), block, 0, st>>>(
                n_rel, ld, cfg, ws, phase == OEA_PHASE_APPLY);
    }
    return 0;
}

}  // namespace

bool oea::apply_g16(int64_t n_ent, int64_t n_rel, int32_t ld) {
    static const int env_g16 = [] { const char *e = getenv("OEA_APPLY_G16"); return e ? atoi(e) : -1; }();
    return env_g16 >= 0 ? env_g16 != 0 : (n_ent + n_rel) * (int64_t)ld * 12 > (int64_t)128 << 20;   // 3 arrays > 128 MB
}

void oea::step_scratch_rows(void *workspace, int64_t n_ent, int64_t n_rel, int32_t ld, grad_t **ent_grad, flag_t **ent_touched,
                            grad_t **rel_grad, flag_t **rel_touched) {
    StepWs ws;
    ws_layout(n_ent, n_rel, ld, workspace, &ws);
    *ent_grad = ws.ent_grad; *ent_touched = ws.ent_touched; *rel_grad = ws.rel_grad; *rel_touched = ws.rel_touched;
}

extern "C" {

size_t oea_step_workspace_bytes(int64_t n_ent, int64_t n_rel, int32_t ld) {
    return ws_layout(n_ent, n_rel, ld, nullptr, nullptr);
}

size_t oea_step_exchange_floats(int64_t n_ent, int64_t n_rel, int32_t ld) {
    StepWs ws;
    ws_layout(n_ent, n_rel, ld, reinterpret_cast<void *>(256), &ws);   // fake base: only offsets matter
    return (size_t)(reinterpret_cast<char *>(ws.rel_extra) - reinterpret_cast<char *>(256)) / sizeof(grad_t);
}

int32_t oea_step_scratch_elem_bytes(void) { return (int32_t)sizeof(grad_t); }

}  // extern "C"

int oea::step_phase_planned(float *ent, float *ent_acc, int64_t n_ent, float *rel, float *rel_acc,
                            int64_t n_rel, int32_t dim, int32_t ld, const int32_t *pos, int64_t n_pos,
                            const int32_t *neg, int64_t n_neg, const oea_step_cfg *cfg, void *workspace,
                            double *loss_accum, int32_t phase, void *stream, const oea::StepPlanView *plan, int plan_step,
                            int64_t plan_first_pos) {
    OEA_REQUIRE(phase >= OEA_PHASE_BOTH && phase <= OEA_PHASE_APPLY, "phase");
    OEA_REQUIRE(ent && rel && (pos || n_pos == 0) && cfg && workspace && loss_accum, "null pointer");
    OEA_REQUIRE(ld % 4 == 0 && dim <= ld && dim > 0, "ld % 4 == 0 and dim <= ld");
    OEA_REQUIRE(n_pos >= 0 && n_neg >= 0 && (neg || n_neg == 0), "neg == NULL needs n_neg == 0");
    OEA_REQUIRE(cfg->loss_kind >= OEA_LOSS_MARGIN && cfg->loss_kind <= OEA_LOSS_ALIGN, "loss_kind");
    OEA_REQUIRE(cfg->opt_kind >= OEA_OPT_SGD && cfg->opt_kind <= OEA_OPT_ADADELTA, "opt_kind");
    OEA_REQUIRE(cfg->opt_kind == OEA_OPT_SGD || phase == OEA_PHASE_GRAD || (ent_acc && rel_acc),
                "Adagrad / Adam / Adadelta need their state arrays (the GRAD phase alone does not)");
    if (cfg->opt_kind == OEA_OPT_ADAM || cfg->opt_kind == OEA_OPT_ADADELTA) {
        OEA_REQUIRE(cfg->score_kind != OEA_SCORE_TRANSH, "Adam / Adadelta are not built for the TransH normal-vector table");
        OEA_REQUIRE(cfg->opt_kind != OEA_OPT_ADAM || cfg->opt_t >= 1, "Adam: opt_t = 1-based step count");
        OEA_REQUIRE(cfg->beta1 > 0.f && cfg->beta1 < 1.f && cfg->eps > 0.f, "beta1 / eps");
    }
    if (cfg->loss_kind == OEA_LOSS_MARGIN) OEA_REQUIRE(n_neg == n_pos, "margin loss pairs pos i with neg i");
    if (cfg->loss_kind == OEA_LOSS_POSITIVE || cfg->loss_kind == OEA_LOSS_ALIGN)
        OEA_REQUIRE(n_neg == 0, "positive-only loss takes no negatives");
    OEA_REQUIRE(cfg->neg_group_k >= 0 && (cfg->neg_group_k == 0 || n_neg == n_pos * (int64_t)cfg->neg_group_k),
                "neg_group_k > 0 needs n_neg == n_pos * neg_group_k");
    OEA_REQUIRE(cfg->score_kind >= OEA_SCORE_TRANSE && cfg->score_kind <= OEA_SCORE_TRANSD, "score_kind");
    if (cfg->score_kind == OEA_SCORE_TRANSH)
        OEA_REQUIRE(cfg->normal && (cfg->opt_kind != OEA_OPT_ADAGRAD || cfg->normal_acc), "TransH needs the normal_vector table (+ accumulator)");
    if (cfg->score_kind == OEA_SCORE_TRANSD)
        OEA_REQUIRE(cfg->ent_transfer_base > 0 && cfg->rel_transfer_base > 0 && 2 * (int64_t)cfg->ent_transfer_base == n_ent &&
                        2 * (int64_t)cfg->rel_transfer_base == n_rel,
                    "TransD: the tables hold the embeddings in rows [0, base) and the transfer vectors in [base, 2 base)");
    if (n_pos + n_neg == 0 && phase != OEA_PHASE_APPLY) return OEA_OK;   // apply-only: externally scattered gradients
    StepWs ws;
    ws_layout(n_ent, n_rel, ld, workspace, &ws);
    hipStream_t st = oea::as_stream(stream);
    int rc_step = OEA_OK;            // launch_step's own refusal (a plan for a width no planned kernel is built for)
    OEA_TRY_RC(for_row_width(ld, [&](auto g, auto it) {
        rc_step = launch_step<decltype(g)::value, decltype(it)::value>(ent, ent_acc, n_ent, rel, rel_acc, n_rel, ld, pos, n_pos, neg, n_neg,
                                                                       *cfg, ws, loss_accum, phase, st, plan, plan_step, plan_first_pos);
    }));
    OEA_TRY_RC(rc_step);
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

extern "C" {

int oea_triple_step_phase(float *ent, float *ent_acc, int64_t n_ent, float *rel, float *rel_acc,
                          int64_t n_rel, int32_t dim, int32_t ld, const int32_t *pos, int64_t n_pos,
                          const int32_t *neg, int64_t n_neg, const oea_step_cfg *cfg, void *workspace,
                          double *loss_accum, int32_t phase, void *stream) {
    return oea::step_phase_planned(ent, ent_acc, n_ent, rel, rel_acc, n_rel, dim, ld, pos, n_pos, neg, n_neg, cfg, workspace, loss_accum,
                                   phase, stream, nullptr, 0, 0);
}

int oea_triple_step(float *ent, float *ent_acc, int64_t n_ent, float *rel, float *rel_acc,
                    int64_t n_rel, int32_t dim, int32_t ld, const int32_t *pos, int64_t n_pos,
                    const int32_t *neg, int64_t n_neg, const oea_step_cfg *cfg, void *workspace,
                    double *loss_accum, void *stream) {
    return oea_triple_step_phase(ent, ent_acc, n_ent, rel, rel_acc, n_rel, dim, ld, pos, n_pos, neg, n_neg, cfg,
                                 workspace, loss_accum, OEA_PHASE_BOTH, stream);
}

int oea_step_entity_scratch(void *workspace, int64_t n_ent, int64_t n_rel, int32_t ld, void **ent_grad, void **ent_touched) {
    OEA_REQUIRE(workspace && ent_grad && ent_touched, "null pointer");
    StepWs ws;
    ws_layout(n_ent, n_rel, ld, workspace, &ws);
    *ent_grad = ws.ent_grad;
    *ent_touched = ws.ent_touched;
    return OEA_OK;
}

int oea_step_scatter_ent_rows(void *workspace, int64_t n_ent, int64_t n_rel, int32_t ld, const int32_t *ids,
                              int64_t n, const float *src, int32_t src_ld, void *stream) {
    OEA_REQUIRE(workspace && ids && src && ld % 4 == 0 && src_ld >= ld, "shapes");
    if (n == 0) return OEA_OK;
    StepWs ws;
    ws_layout(n_ent, n_rel, ld, workspace, &ws);
    scatter_rows_kernel<<<(unsigned)std::min<int64_t>(oea::ceil_div(n * ld, 256), 65535), 256, 0, oea::as_stream(stream)>>>(
        ws.ent_grad, ws.ent_touched, ld, ids, n, src, src_ld);
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

/* TransH under the entity-id partition: the normal-vector table is relation-sized and replicated, so its gradient scratch
 * (copy 0 after the GRAD phase folded the copies) and touched flags are summed over the ranks with two small all-reduces
 * and every rank applies the same update.  oea_step_normal_scratch: where the two regions sit in the workspace (byte
 * offsets + float counts); oea_step_apply_normals: the optimiser on the touched normal rows (cfg->normal / normal_acc). */
int oea_step_normal_scratch(int64_t n_ent, int64_t n_rel, int32_t ld, int64_t *grad_offset_bytes, int64_t *touched_offset_bytes) {
    OEA_REQUIRE(grad_offset_bytes && touched_offset_bytes, "null pointer");
    StepWs ws;
    ws_layout(n_ent, n_rel, ld, reinterpret_cast<void *>(256), &ws);           // fake base: only offsets matter
    *grad_offset_bytes = reinterpret_cast<char *>(ws.nrm_grad) - reinterpret_cast<char *>(256);
    *touched_offset_bytes = reinterpret_cast<char *>(ws.nrm_touched) - reinterpret_cast<char *>(256);
    return OEA_OK;
}

int oea_step_apply_normals(int64_t n_ent, int64_t n_rel, int32_t ld, const oea_step_cfg *cfg, void *workspace, void *stream) {
    OEA_REQUIRE(cfg && workspace && ld % 4 == 0, "arguments");
    OEA_REQUIRE(cfg->score_kind == OEA_SCORE_TRANSH && cfg->normal, "TransH score with its normal-vector table");
    OEA_REQUIRE(cfg->opt_kind == OEA_OPT_SGD || (cfg->opt_kind == OEA_OPT_ADAGRAD && cfg->normal_acc), "SGD or Adagrad (+ state)");
    if (n_rel == 0) return OEA_OK;
    StepWs ws;
    ws_layout(n_ent, n_rel, ld, workspace, &ws);
    hipStream_t st = oea::as_stream(stream);
    OEA_TRY_RC(for_row_width(ld, [&](auto g, auto it) {
        constexpr int G = decltype(g)::value;
        apply_normal_rows<G, decltype(it)::value><<<(unsigned)std::max<int64_t>(oea::ceil_div(n_rel, 256 / G), 1), 256, 0, st>>>(n_rel, ld, *cfg, ws, 1);
    }));
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

int64_t oea_step_items(const oea_step_cfg *cfg, int64_t n_pos, int64_t n_neg) { return cfg ? step_items(*cfg, n_pos, n_neg) : -1; }

// 1 when an epoch of this configuration would run on the gathered-sum plan (step_plan.h): triple_wave's rule, SGD / Adagrad, the
// fp32 scratch (the fixed-point build keeps ONE summation path for one GPU and for G ranks), OEA_STEP_PLAN != 0
int32_t oea_step_plan_supported(const oea_step_cfg *cfg, int64_t n_ent, int64_t n_rel, int32_t ld, int32_t k) {
    static const int env = [] { const char *e = getenv("OEA_STEP_PLAN"); return e ? atoi(e) : 1; }();
    if (!cfg || env == 0 || oea::kDetScratch) return 0;
    // tables that fit the caches (the 15K shape: 9 MB) keep the flag-driven optimiser: its streaming pass over the whole table
    // costs 11 us there and the plan's chains of dependent loads 20 (measured, tools/r06/d.sh); OEA_STEP_PLAN=2 forces the plan
    if (env != 2 && !oea::apply_g16(n_ent, n_rel, ld)) return 0;
    return wave_rule(*cfg, n_ent, n_rel, ld) && cfg->neg_group_k == k && (cfg->opt_kind == OEA_OPT_SGD || cfg->opt_kind == OEA_OPT_ADAGRAD);
}

}  // extern "C"

