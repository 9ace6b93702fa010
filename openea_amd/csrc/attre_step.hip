// attre_step.hip -- AttrE's character step, its head-only negative sampler and its joint epoch (approaches/attre.py:88-109, 166-191,
// 221-233 of the reference; modules/train/batch.py:187-199).
//
// Character step.  With ue = l2n?(ent_ce)[e], wa = l2n?(attr)[a] and the value vector composed from the L characters of the triple's
// own value row,
//   v = sum_p w_p l2n?(chars)[id_p],   w_p = sum_{m = p + 1 .. L} 1 / m     (the reference's while_loop over the reversed prefixes),
// the score of (e, a, v) is |x|^2 or |x|_1 of x = ue + wa - v, and the loss is one of losses.py's three over a positive and its k
// head-corrupted negatives (e', a, v).  One wave per positive and its negatives, as jape_kernel: a lane holds columns 2 l and 2 l + 1,
// the entity and attribute gradient rows go through the step engine's scratch (ent_ce = its entity table, attr = its relation table)
// and the engine's apply phase takes them back through the normalisation.  Because a negative keeps a and v, wa and v are formed once
// per positive and with g_q = dL/dx_q:  dL/due_q = g_q,  dL/dwa = sum_q g_q,  dL/dv = gv = -sum_q g_q.
//
// The character table has about a hundred rows and every positive sends L rows to it: float atomics of every adder on a few rows.
// So the wave only STORES gv [n_pos, ld]; char_grad_kernel then forms G[c] = sum_{(p, i): id_{p, i} = c} w_i gv[p]
//   LDS path     a workgroup takes a slice of the positives, adds into a [C, ld] slab in LDS (ds_add) and stores the slab to partials[g];
//   atomic path  (the slab does not fit) row adds into one dense [C, ld] buffer: there the rows are many and the adders spread out;
// and char_apply_kernel sums the partials in a fixed order, goes back through l2n and runs SGD or Adagrad on the C rows.  The slab holds
// grad_t: int64 fixed point in the deterministic build, where the sums then do not depend on the order of the adds.
//
// Joint epoch.  loss = sum_e (1 - l2n?(ent)[e] . l2n?(ent_ce)[e]) over ALL entities in every step: row e's update reads only row e of
// the two tables, so a wave keeps both rows in registers over the S steps of an epoch and stores them once.
#include "common.h"
#include "row_ops.h"

#include <algorithm>

namespace {

using oea::flag_t;
using oea::grad_t;
using namespace oea::row;

constexpr int kMaxDim = 128;
constexpr int kWaves = 4;
constexpr int kGradWaves = 16;                // waves on one LDS slab of the character gradient
constexpr int kMaxBlocks = 2048;
constexpr int kMaxLen = 32;
constexpr int kMaxSlabs = 512;                 // partial slabs of the LDS path
constexpr int kSlabPositives = 16;             // positives a slab takes before another slab is opened: one per wave
constexpr int kSlabBytes = 128 * 1024;         // of the CU's 160 KiB: the rest stays free for the compiler's own and a second small kernel
constexpr int kJointSteps = 32;                // steps of one joint launch (the entry point splits longer epochs)

enum { ERR_CHAR = 1, ERR_ROW = 2 };

struct CharWs {
    float *inv;         // [C] inverse norms of the character rows
    float *w;           // [kMaxLen] composition weights
    float *gv;          // [max_pos, ld]
    grad_t *partials;   // [slabs, C, ld]
};

size_t partial_slabs(int64_t n_chars, int32_t ld) { return (size_t)n_chars * ld * sizeof(grad_t) <= (size_t)kSlabBytes ? kMaxSlabs : 1; }

size_t carve(void *workspace, int64_t n_chars, int32_t ld, int64_t max_pos, CharWs *ws) {
    char *base = static_cast<char *>(workspace);
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = base + off; off += oea::align256(bytes); return p; };
    float *inv = reinterpret_cast<float *>(take((size_t)n_chars * sizeof(float)));
    float *w = reinterpret_cast<float *>(take(kMaxLen * sizeof(float)));
    float *gv = reinterpret_cast<float *>(take((size_t)max_pos * ld * sizeof(float)));
    grad_t *partials = reinterpret_cast<grad_t *>(take(partial_slabs(n_chars, ld) * (size_t)n_chars * ld * sizeof(grad_t)));
    if (ws) { ws->inv = inv; ws->w = w; ws->gv = gv; ws->partials = partials; }
    return off;
}

// ---- prologue: inverse norms of the C rows, the weights, and the checks of every id the step will index with --------------------
__global__ __launch_bounds__(64 * kWaves) void prologue_kernel(const float *chars, int64_t n_chars, int ld, int dim, int char_l2n,
                                                                float *inv, float *w, const int32_t *value_chars, int64_t n_values,
                                                                int len, const int32_t *pos, const int32_t *neg_heads, int64_t n_pos, int k,
                                                                int64_t n_ent, int64_t n_attr, int32_t *err_flag) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t c = (int64_t)blockIdx.x * kWaves + wave; c < n_chars; c += (int64_t)gridDim.x * kWaves) {
        const float2 a = load2(chars + c * ld, dim, lane);
        const float s = inv_norm(a, char_l2n);
        if (lane == 0) inv[c] = s;
    }
    if (blockIdx.x == 0 && threadIdx.x < len) {
        double s = 0.0;
        for (int m = threadIdx.x + 1; m <= len; ++m) s += 1.0 / (double)m;
        w[threadIdx.x] = (float)s;
    }
    int bad = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = t0; i < n_pos * len; i += stride) {
        const int32_t v = pos[3 * (i / len) + 2];
        if (v < 0 || v >= n_values) {
            bad |= ERR_ROW;
        } else {
            const int32_t c = value_chars[(int64_t)v * len + i % len];
            if (c < 0 || c >= n_chars) bad |= ERR_CHAR;
        }
    }
    for (int64_t p = t0; p < n_pos; p += stride) {
        const int32_t e = pos[3 * p], a = pos[3 * p + 1];
        if (e < 0 || e >= n_ent || a < 0 || a >= n_attr) bad |= ERR_ROW;
    }
    for (int64_t i = t0; i < n_pos * k; i += stride) {
        const int32_t e = neg_heads[i];
        if (e < 0 || e >= n_ent) bad |= ERR_ROW;
    }
    if (bad) atomicOr(err_flag, bad);
}

// ---- the scoring kernel ------------------------------------------------------------------------------------------------------------
struct CharArgs {
    const float *ent, *attr, *chars, *inv, *w;
    int ld, dim, len, k;
    const int32_t *value_chars, *pos, *neg_heads;
    int64_t n_pos;
    int loss_kind, l1;
    float margin, pos_margin, neg_margin, balance;
    int ent_l2n, attr_l2n;
    grad_t *ent_grad, *attr_grad;
    flag_t *ent_touched, *attr_touched;
    float *gv;
    const int32_t *err_flag;
    double *loss_accum;
};

__device__ __forceinline__ float score_of(float2 x, int l1) { return l1 ? oea::group_sum<64>(fabsf(x.x) + fabsf(x.y)) : dot2(x, x); }
__device__ __forceinline__ float sign_f(float x) { return (float)(x > 0.f) - (float)(x < 0.f); }
// c d score / d x
__device__ __forceinline__ float2 score_grad(float2 x, int l1, float c) {
    return l1 ? make_float2(c * sign_f(x.x), c * sign_f(x.y)) : scale2(x, 2.f * c);
}

__global__ __launch_bounds__(64 * kWaves) void char_kernel(CharArgs A) {
    __shared__ __attribute__((aligned(16))) float buf[kWaves][kMaxDim];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = A.k, l1 = A.l1;
    const bool refused = *A.err_flag != 0;                  // every thread reads the same word: the block stays together
    double loss_local = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * kWaves + wave; !refused && p < A.n_pos; p += (int64_t)gridDim.x * kWaves) {
        const int32_t *tp = A.pos + 3 * p;
        const int64_t e = tp[0], a = tp[1], vid = tp[2];
        const int32_t my_id = lane < A.len ? A.value_chars[vid * A.len + lane] : 0;
        const float my_scale = lane < A.len ? A.w[lane] * A.inv[my_id] : 0.f;       // lane i: w_i / |char row of id_i|
        float2 val = make_float2(0.f, 0.f);
        for (int i = 0; i < A.len; ++i) {
            const int64_t c = __shfl(my_id, i, 64);
            val = add2(val, scale2(load2(A.chars + c * A.ld, A.dim, lane), __shfl(my_scale, i, 64)));
        }
        const float2 ar = load2(A.attr + a * A.ld, A.dim, lane);
        const float2 wa = scale2(ar, inv_norm(ar, A.attr_l2n));
        const float2 er = load2(A.ent + e * A.ld, A.dim, lane);
        const float2 ue = scale2(er, inv_norm(er, A.ent_l2n));
        const float2 x0 = make_float2(ue.x + wa.x - val.x, ue.y + wa.y - val.y);
        Slots<1> se;
        se.set(0, e);
        float2 gsum = make_float2(0.f, 0.f);
        bool any = false;
        if (A.loss_kind == OEA_LOSS_MARGIN) {                 // k == 1: relu(margin + pos - neg)
            const int64_t e1 = A.neg_heads[p];
            const float2 nr = load2(A.ent + e1 * A.ld, A.dim, lane);
            const float2 un = scale2(nr, inv_norm(nr, A.ent_l2n));
            const float2 x1 = make_float2(un.x + wa.x - val.x, un.y + wa.y - val.y);
            const float l = A.margin + score_of(x0, l1) - score_of(x1, l1);
            if (l > 0.f) {                                    // a hinge at exactly zero gives no gradient
                loss_local += (double)l;
                const float2 g0 = score_grad(x0, l1, 1.f), g1 = score_grad(x1, l1, -1.f);
                se.add(e, g0, A.ent_grad, A.ent_touched, A.ld, A.dim, lane, buf[wave]);
                se.add(e1, g1, A.ent_grad, A.ent_touched, A.ld, A.dim, lane, buf[wave]);
                gsum = add2(g0, g1);
                any = true;
            }
        } else {
            for (int q = 0; q <= k; ++q) {
                float2 x = x0;
                int64_t eq = e;
                if (q > 0) {
                    eq = A.neg_heads[p * k + q - 1];
                    const float2 nr = load2(A.ent + eq * A.ld, A.dim, lane);
                    const float2 un = scale2(nr, inv_norm(nr, A.ent_l2n));
                    x = make_float2(un.x + wa.x - val.x, un.y + wa.y - val.y);
                }
                const float s = score_of(x, l1);
                float c;
                if (A.loss_kind == OEA_LOSS_LOGISTIC) {       // log(1 + e^pos), log(1 + e^-neg)
                    loss_local += (double)softplus_f(q == 0 ? s : -s);
                    c = q == 0 ? sigmoid_f(s) : -sigmoid_f(-s);
                } else {                                      // limited: relu(pos - pos_margin), balance relu(neg_margin - neg)
                    const float d = q == 0 ? s - A.pos_margin : A.neg_margin - s;
                    const float wgt = q == 0 ? 1.f : A.balance;
                    loss_local += (double)(wgt * fmaxf(d, 0.f));
                    c = d > 0.f ? (q == 0 ? 1.f : -A.balance) : 0.f;
                }
                if (c != 0.f) {
                    const float2 g = score_grad(x, l1, c);
                    se.add(eq, g, A.ent_grad, A.ent_touched, A.ld, A.dim, lane, buf[wave]);
                    gsum = add2(gsum, g);
                    any = true;
                }
            }
        }
        if (any) {
            se.flush(A.ent_grad, A.ent_touched, A.ld, A.dim, lane, buf[wave]);
            flush_row(A.attr_grad, A.attr_touched, a, gsum, A.ld, A.dim, lane, buf[wave]);
        }
        if (2 * lane < A.ld) *reinterpret_cast<float2 *>(A.gv + p * A.ld + 2 * lane) = make_float2(-gsum.x, -gsum.y);
    }
    oea::block_loss_add<kWaves>(loss_local, lane, wave, A.loss_accum);
}

// ---- G[c] = sum w_i gv[p] over the batch's (p, i) with id = c ------------------------------------------------------------------------
#ifdef OEA_DET_SCRATCH
__device__ __forceinline__ void lds_add(grad_t *p, float v) {
    atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)oea::to_fixed(v));
}
#else
__device__ __forceinline__ void lds_add(grad_t *p, float v) { atomicAdd(p, v); }
#endif

// LDS: block g takes positives [g per_slab, (g + 1) per_slab) and writes out + g C ld; otherwise a grid-stride walk that adds into out.
// A positive is a chain of dependent loads (its value row, then the row's ids), so the LDS form runs kGradWaves waves on one slab:
// the waves hide each other's loads and the number of partials stays small.
template <bool LDS>
__global__ __launch_bounds__(64 * kGradWaves) void char_grad_kernel(const float *gv, const int32_t *pos, const int32_t *value_chars, const float *w,
                                                                 int64_t n_pos, int len, int ld, int dim, int64_t n_chars, int64_t per_slab,
                                                                 grad_t *out, const int32_t *err_flag) {
    extern __shared__ __attribute__((aligned(16))) unsigned char slab_raw[];
    grad_t *slab = reinterpret_cast<grad_t *>(slab_raw);
    if (*err_flag != 0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int64_t cells = n_chars * ld;
    const float my_w = lane < len ? w[lane] : 0.f;          // lane i holds w_i: no load inside the loop over the characters
    int64_t p0 = (int64_t)blockIdx.x * waves + wave, p1 = n_pos, step = (int64_t)gridDim.x * waves;
    if (LDS) {
        for (int64_t i = threadIdx.x; i < cells; i += blockDim.x) slab[i] = 0;
        __syncthreads();
        p0 = (int64_t)blockIdx.x * per_slab + wave;
        p1 = ((int64_t)blockIdx.x + 1) * per_slab < n_pos ? ((int64_t)blockIdx.x + 1) * per_slab : n_pos;
        step = waves;
    }
    for (int64_t p = p0; p < p1; p += step) {
        const int64_t vid = pos[3 * p + 2];
        const int32_t my_id = lane < len ? value_chars[vid * len + lane] : 0;
        const float g0 = lane < dim ? gv[p * ld + lane] : 0.f, g1 = lane + 64 < dim ? gv[p * ld + lane + 64] : 0.f;
        for (int i = 0; i < len; ++i) {
            const int64_t c = __shfl(my_id, i, 64);
            const float wi = __shfl(my_w, i, 64);
            grad_t *row = (LDS ? slab : out) + c * ld;
            if (LDS) {
                if (lane < dim) lds_add(row + lane, wi * g0);
                if (lane + 64 < dim) lds_add(row + lane + 64, wi * g1);
            } else {
                if (lane < dim) oea::grad_add(row + lane, wi * g0);
                if (lane + 64 < dim) oea::grad_add(row + lane + 64, wi * g1);
            }
        }
    }
    if (LDS) {
        __syncthreads();
        grad_t *dst = out + (int64_t)blockIdx.x * cells;
        for (int64_t i = threadIdx.x; i < cells; i += blockDim.x) dst[i] = slab[i];
    }
}

// back through the normalisation and one optimiser step on a row held as columns 2 l, 2 l + 1 (apply_one_row of step_rows.h)
__device__ __forceinline__ float2 through_l2n(float2 r, float2 g, int on) {
    if (!on) return g;
    const float ss = dot2(r, r);
    const float inv = rsqrtf(fmaxf(ss, 1e-12f));
    const float dot = dot2(r, g) * inv;
    const float ydg = ss > 1e-12f ? dot : 0.f;
    return make_float2((g.x - r.x * inv * ydg) * inv, (g.y - r.y * inv * ydg) * inv);
}
__device__ __forceinline__ void optimiser(float2 &r, float2 &acc, float2 g, int adagrad, float lr) {
    if (adagrad) {
        acc = make_float2(acc.x + g.x * g.x, acc.y + g.y * g.y);
        r = make_float2(r.x - lr * g.x / sqrtf(acc.x), r.y - lr * g.y / sqrtf(acc.y));
    } else {
        r = make_float2(r.x - lr * g.x, r.y - lr * g.y);
    }
}
// an Adagrad accumulator row; the columns from dim on read as 1 so that 0 / sqrt(acc) stays 0 there (a row kept in registers over
// several steps must not pick up a NaN in its pad columns)
__device__ __forceinline__ float2 load2_acc(const float *row, int dim, int lane) {
    float2 v = load2(row, dim, lane);
    if (2 * lane >= dim) v.x = 1.f;
    if (2 * lane + 1 >= dim) v.y = 1.f;
    return v;
}
__device__ __forceinline__ void store2(float *row, float2 v, int dim, int lane) {
    const int c = 2 * lane;
    if (c + 1 < dim) *reinterpret_cast<float2 *>(row + c) = v;
    else if (c < dim) row[c] = v.x;
}

// one workgroup per character row: its waves sum a quarter of the partials each, wave 0 adds the quarters in wave order (a fixed order;
// exact in the fixed-point build), goes back through the normalisation and runs the optimiser
__global__ __launch_bounds__(64 * kWaves) void char_apply_kernel(float *chars, float *acc, int64_t n_chars, int ld, int dim, int l2n,
                                                                  const grad_t *partials, int n_part, int adagrad, float lr,
                                                                  const int32_t *err_flag) {
    __shared__ grad_t quarter[kWaves][kMaxDim];
    if (*err_flag != 0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t cells = n_chars * ld;
    const int per = (n_part + kWaves - 1) / kWaves;
    const int g0 = wave * per, g1 = g0 + per < n_part ? g0 + per : n_part;
    for (int64_t c = blockIdx.x; c < n_chars; c += gridDim.x) {
        grad_t q0 = 0, q1 = 0;
        if (2 * lane < dim) {
            const grad_t *src = partials + c * ld + 2 * lane;
#pragma unroll 4
            for (int g = g0; g < g1; ++g) {
                q0 += src[g * cells];
                q1 += src[g * cells + 1];
            }
        }
        quarter[wave][2 * lane] = q0;
        quarter[wave][2 * lane + 1] = q1;
        __syncthreads();
        if (wave == 0) {
            q0 = quarter[0][2 * lane];
            q1 = quarter[0][2 * lane + 1];
            for (int w = 1; w < kWaves; ++w) {
                q0 += quarter[w][2 * lane];
                q1 += quarter[w][2 * lane + 1];
            }
            float2 g = make_float2(2 * lane < dim ? oea::grad_val(q0) : 0.f, 2 * lane + 1 < dim ? oea::grad_val(q1) : 0.f);
            float2 r = load2(chars + c * ld, dim, lane);
            float2 a = adagrad ? load2_acc(acc + c * ld, dim, lane) : make_float2(1.f, 1.f);
            g = through_l2n(r, g, l2n);
            optimiser(r, a, g, adagrad, lr);
            store2(chars + c * ld, r, dim, lane);
            if (adagrad) store2(acc + c * ld, a, dim, lane);
        }
        __syncthreads();
    }
}

// ---- head-only negatives ------------------------------------------------------------------------------------------------------------
struct HeadSide {
    const int32_t *list, *ent_pos;
    int32_t n;
};

__global__ __launch_bounds__(256) void sample_heads_kernel(const int32_t *pos, int64_t n_pos, int64_t n_split, int k, HeadSide s0, HeadSide s1,
                                                            int64_t n_ent, uint32_t k0, uint32_t k1, uint32_t step, uint32_t pos_offset,
                                                            int32_t *out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pos * k) return;
    const int64_t p = i / k;
    const uint32_t s = (uint32_t)(i % k);
    const HeadSide sd = p < n_split ? s0 : s1;
    const int32_t h = pos[3 * p];
    const int32_t own = h >= 0 && h < n_ent ? sd.ent_pos[h] : -1;
    const bool listed = own >= 0 && own < sd.n;
    const uint4 r = oea::philox4x32_10((uint32_t)p + pos_offset, step, 0u, s, k0, k1);
    uint32_t j = __umulhi(r.x, (uint32_t)(listed ? sd.n - 1 : sd.n));       // uniform over the list without the head's own position
    if (listed && j >= (uint32_t)own) ++j;
    out[i] = sd.list[j];
}

// ---- joint epoch ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * kWaves) void joint_kernel(float *ent, float *ent_acc, float *ce, float *ce_acc, const int32_t *row_count,
                                                             int64_t n_ent, int ld, int dim, int l2n, int adagrad, float lr, int steps,
                                                             double *loss_accum) {
    __shared__ double wave_loss[kWaves][kJointSteps];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane < steps) wave_loss[wave][lane] = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * kWaves + wave; e < n_ent; e += (int64_t)gridDim.x * kWaves) {
        const int32_t times = row_count ? row_count[e] : 1;       // how often the step's entity list names the row
        if (times <= 0) continue;
        const float m = (float)times;
        float2 a = load2(ent + e * ld, dim, lane), b = load2(ce + e * ld, dim, lane);
        float2 aa = make_float2(1.f, 1.f), ba = aa;
        if (adagrad) { aa = load2_acc(ent_acc + e * ld, dim, lane); ba = load2_acc(ce_acc + e * ld, dim, lane); }
        for (int s = 0; s < steps; ++s) {
            // three wave sums a step: the two norms and the cosine.  The gradient w.r.t. ya is -m yb, so the y . g of the way back
            // through the normalisation is -m cs (and 0 for a clamped row, as apply_one_row of step_rows.h has it)
            float ia = 1.f, ib = 1.f, pa = 0.f, pb = 0.f;
            if (l2n) {
                const float sa = dot2(a, a), sb = dot2(b, b);
                ia = rsqrtf(fmaxf(sa, 1e-12f));
                ib = rsqrtf(fmaxf(sb, 1e-12f));
                pa = sa > 1e-12f ? 1.f : 0.f;
                pb = sb > 1e-12f ? 1.f : 0.f;
            }
            const float2 ya = scale2(a, ia), yb = scale2(b, ib);
            const float cs = dot2(ya, yb);
            if (lane == 0) wave_loss[wave][s] += (double)times * (1.0 - (double)cs);
            const float ca = m * cs * pa, cb = m * cs * pb;
            const float2 ga = make_float2((ya.x * ca - m * yb.x) * ia, (ya.y * ca - m * yb.y) * ia);
            const float2 gb = make_float2((yb.x * cb - m * ya.x) * ib, (yb.y * cb - m * ya.y) * ib);
            optimiser(a, aa, ga, adagrad, lr);
            optimiser(b, ba, gb, adagrad, lr);
        }
        store2(ent + e * ld, a, dim, lane);
        store2(ce + e * ld, b, dim, lane);
        if (adagrad) { store2(ent_acc + e * ld, aa, dim, lane); store2(ce_acc + e * ld, ba, dim, lane); }
    }
    __syncthreads();
    if (threadIdx.x < steps) {
        double s = 0.0;
        for (int w = 0; w < kWaves; ++w) s += wave_loss[w][threadIdx.x];
        if (s != 0.0) atomicAdd(loss_accum + threadIdx.x, s);
    }
}

// CUs of the current device, at most kMaxSlabs (256 on an MI355X); 64 if the runtime does not say
int compute_units() {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 64;
    return std::min(n, kMaxSlabs);
}

int unsupported_optimiser(const char *who, int kind) {
    if (kind == OEA_OPT_SGD || kind == OEA_OPT_ADAGRAD) return 0;
    oea::set_error("%s: optimizer %d (SGD or Adagrad only)", who, kind);
    return OEA_EUNSUPPORTED;
}

}  // namespace

extern "C" {

int64_t oea_attre_lds_chars(int32_t ld) { return ld > 0 ? (int64_t)kSlabBytes / ((int64_t)ld * (int64_t)sizeof(grad_t)) : 0; }

size_t oea_attre_char_workspace_bytes(int64_t n_chars, int32_t ld, int64_t max_pos) {
    if (n_chars < 1 || ld < 1 || max_pos < 0) return 0;
    return carve(nullptr, n_chars, ld, max_pos, nullptr);
}

int oea_attre_char_step(float *ent_ce, float *ent_acc, int64_t n_ent, float *attr, float *attr_acc, int64_t n_attr, float *chars,
                        float *char_acc, int64_t n_chars, int32_t dim, int32_t ld, const int32_t *value_chars, int64_t n_values,
                        int32_t literal_len, const int32_t *pos, int64_t n_pos, const int32_t *neg_heads, int64_t n_neg,
                        int32_t char_l2_norm, int32_t char_path, int32_t n_slabs, const oea_step_cfg *cfg, void *step_workspace,
                        void *char_workspace, size_t char_workspace_bytes, int32_t *err_flag, double *loss_accum, void *stream) {
    OEA_REQUIRE(ent_ce && attr && chars && value_chars && cfg && step_workspace && char_workspace && err_flag && loss_accum, "null pointer");
    OEA_REQUIRE(n_pos >= 0 && (pos || n_pos == 0) && (neg_heads || n_neg == 0), "pos / neg_heads");
    OEA_REQUIRE(n_ent >= 1 && n_attr >= 1 && n_chars >= 1 && n_values >= 1, "table rows");
    if (int rc = unsupported_optimiser("oea_attre_char_step", cfg->opt_kind)) return rc;
    OEA_REQUIRE(cfg->opt_kind == OEA_OPT_SGD || (ent_acc && attr_acc && char_acc), "Adagrad needs its three accumulators");
    OEA_REQUIRE(cfg->score_kind == OEA_SCORE_TRANSE, "cfg: score_kind OEA_SCORE_TRANSE");
    OEA_REQUIRE(cfg->loss_kind == OEA_LOSS_MARGIN || cfg->loss_kind == OEA_LOSS_LIMITED || cfg->loss_kind == OEA_LOSS_LOGISTIC,
                "cfg: loss_kind margin-based, limited or logistic");
    const int64_t k = cfg->neg_group_k;
    OEA_REQUIRE(k >= 1 && n_neg == k * n_pos, "neg_group_k = k >= 1 and n_neg == k n_pos (neg_heads[p k .. p k + k) corrupt pos p)");
    OEA_REQUIRE(cfg->loss_kind != OEA_LOSS_MARGIN || k == 1, "margin-based: k == 1 (pairs aligned, losses.py:26)");
    OEA_REQUIRE(ld % 4 == 0, "ld % 4 == 0");
    OEA_REQUIRE(dim > 0 && dim <= ld, "0 < dim <= ld");
    OEA_REQUIRE(literal_len >= 1 && literal_len <= kMaxLen, "1 <= literal_len <= 32");
    OEA_REQUIRE(char_path >= 0 && char_path <= 2 && n_slabs >= 0 && n_slabs <= kMaxSlabs, "char_path in 0..2, n_slabs in 0..512");
    if (dim > kMaxDim) {
        oea::set_error("oea_attre_char_step: dim %d > %d", dim, kMaxDim);
        return OEA_EUNSUPPORTED;
    }
    const bool fits = n_chars <= oea_attre_lds_chars(ld);
    OEA_REQUIRE(char_path != 1 || fits, "char_path 1: the [n_chars, ld] slab does not fit (oea_attre_lds_chars)");
    OEA_REQUIRE(char_workspace_bytes >= carve(nullptr, n_chars, ld, n_pos, nullptr), "char_workspace too small (oea_attre_char_workspace_bytes)");
    const bool lds = char_path == 1 || (char_path == 0 && fits);
    const size_t slab_bytes = (size_t)n_chars * ld * sizeof(grad_t);
    if (lds && slab_bytes > 48 * 1024) {
        static const hipError_t attr_rc = hipFuncSetAttribute(reinterpret_cast<const void *>(&char_grad_kernel<true>),
                                                              hipFuncAttributeMaxDynamicSharedMemorySize, kSlabBytes);
        OEA_CHECK_HIP(attr_rc);
    }
    hipStream_t st = oea::as_stream(stream);
    if (n_pos > 0) {
        CharWs ws;
        carve(char_workspace, n_chars, ld, n_pos, &ws);
        const int adagrad = cfg->opt_kind == OEA_OPT_ADAGRAD;
        const unsigned grid = (unsigned)std::min<int64_t>(oea::ceil_div(n_pos, kWaves), kMaxBlocks);
        prologue_kernel<<<grid, 64 * kWaves, 0, st>>>(chars, n_chars, ld, dim, char_l2_norm, ws.inv, ws.w, value_chars, n_values, literal_len,
                                                      pos, neg_heads, n_pos, (int)k, n_ent, n_attr, err_flag);
        OEA_CHECK_HIP(hipGetLastError());
        CharArgs A;
        A.ent = ent_ce; A.attr = attr; A.chars = chars; A.inv = ws.inv; A.w = ws.w;
        A.ld = ld; A.dim = dim; A.len = literal_len; A.k = (int)k;
        A.value_chars = value_chars; A.pos = pos; A.neg_heads = neg_heads; A.n_pos = n_pos;
        A.loss_kind = cfg->loss_kind; A.l1 = cfg->l1;
        A.margin = cfg->margin; A.pos_margin = cfg->pos_margin; A.neg_margin = cfg->neg_margin; A.balance = cfg->balance;
        A.ent_l2n = cfg->ent_l2_norm; A.attr_l2n = cfg->rel_l2_norm;
        oea::step_scratch_rows(step_workspace, n_ent, n_attr, ld, &A.ent_grad, &A.ent_touched, &A.attr_grad, &A.attr_touched);
        A.gv = ws.gv; A.err_flag = err_flag; A.loss_accum = loss_accum;
        char_kernel<<<grid, 64 * kWaves, 0, st>>>(A);
        OEA_CHECK_HIP(hipGetLastError());
        int n_part = 1;
        if (lds) {
            // measured (tools/attre_step_time.py): the LDS adds of a slab run at one CU's rate, so the time falls with the number of
            // slabs up to one per CU and rises beyond (two slabs share a CU's LDS; the closing kernel reads more partials)
            n_part = n_slabs > 0 ? n_slabs : (int)std::min<int64_t>(oea::ceil_div(n_pos, kSlabPositives), compute_units());
            const int64_t per_slab = oea::ceil_div(n_pos, n_part);
            n_part = (int)oea::ceil_div(n_pos, per_slab);
            char_grad_kernel<true><<<n_part, 64 * kGradWaves, slab_bytes, st>>>(ws.gv, pos, value_chars, ws.w, n_pos, literal_len, ld, dim, n_chars,
                                                                            per_slab, ws.partials, err_flag);
        } else {
            OEA_CHECK_HIP(hipMemsetAsync(ws.partials, 0, slab_bytes, st));
            char_grad_kernel<false><<<grid, 64 * kWaves, 0, st>>>(ws.gv, pos, value_chars, ws.w, n_pos, literal_len, ld, dim, n_chars, 0,
                                                                  ws.partials, err_flag);
        }
        OEA_CHECK_HIP(hipGetLastError());
        const unsigned cgrid = (unsigned)std::min<int64_t>(n_chars, kMaxBlocks);
        char_apply_kernel<<<cgrid, 64 * kWaves, 0, st>>>(chars, char_acc, n_chars, ld, dim, char_l2_norm, ws.partials, n_part, adagrad, cfg->lr,
                                                         err_flag);
        OEA_CHECK_HIP(hipGetLastError());
    }
    return oea_triple_step_phase(ent_ce, ent_acc, n_ent, attr, attr_acc, n_attr, dim, ld, nullptr, 0, nullptr, 0, cfg, step_workspace,
                                 loss_accum, OEA_PHASE_APPLY, stream);
}

int oea_attre_sample_heads(const int32_t *pos, int64_t n_pos, int64_t n_split, int32_t k, const int32_t *entity_list0, int32_t n_ent_list0,
                           const int32_t *ent_pos0, const int32_t *entity_list1, int32_t n_ent_list1, const int32_t *ent_pos1,
                           int64_t n_ent, uint64_t seed, uint32_t step, uint32_t pos_offset, int32_t *out, void *stream) {
    OEA_REQUIRE(n_pos >= 0 && k >= 1 && n_split >= 0 && n_split <= n_pos, "n_pos >= 0, k >= 1, 0 <= n_split <= n_pos");
    OEA_REQUIRE((pos && out) || n_pos == 0, "null pointer");
    OEA_REQUIRE(n_split == 0 || (entity_list0 && ent_pos0), "side 0: null pointer");
    OEA_REQUIRE(n_split == n_pos || (entity_list1 && ent_pos1), "side 1: null pointer");
    OEA_REQUIRE(n_split == 0 || n_ent_list0 >= 2, "side 0: n_ent_list < 2 (no other head to draw)");
    OEA_REQUIRE(n_split == n_pos || n_ent_list1 >= 2, "side 1: n_ent_list < 2 (no other head to draw)");
    OEA_REQUIRE(n_ent >= 1 && n_pos * (int64_t)k < ((int64_t)1 << 31), "n_ent >= 1, n_pos k < 2^31");
    if (n_pos == 0) return OEA_OK;
    const HeadSide s0{entity_list0, ent_pos0, n_ent_list0}, s1{entity_list1, ent_pos1, n_ent_list1};
    sample_heads_kernel<<<(unsigned)oea::ceil_div(n_pos * k, 256), 256, 0, oea::as_stream(stream)>>>(
        pos, n_pos, n_split, k, s0, s1, n_ent, (uint32_t)seed, (uint32_t)(seed >> 32), step, pos_offset, out);
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

int oea_attre_joint_epoch(float *ent, float *ent_acc, float *ent_ce, float *ent_ce_acc, const int32_t *row_count, int64_t n_ent, int32_t dim,
                          int32_t ld, int32_t ent_l2_norm, int32_t opt_kind, float lr, int32_t steps, double *loss_accum, void *stream) {
    OEA_REQUIRE(ent && ent_ce && loss_accum, "null pointer");
    if (int rc = unsupported_optimiser("oea_attre_joint_epoch", opt_kind)) return rc;
    OEA_REQUIRE(opt_kind == OEA_OPT_SGD || (ent_acc && ent_ce_acc), "Adagrad needs its two accumulators");
    OEA_REQUIRE(n_ent >= 1 && steps >= 1, "n_ent >= 1, steps >= 1");
    OEA_REQUIRE(ld % 4 == 0, "ld % 4 == 0");
    OEA_REQUIRE(dim > 0 && dim <= ld, "0 < dim <= ld");
    if (dim > kMaxDim) {
        oea::set_error("oea_attre_joint_epoch: dim %d > %d", dim, kMaxDim);
        return OEA_EUNSUPPORTED;
    }
    const unsigned grid = (unsigned)std::min<int64_t>(oea::ceil_div(n_ent, kWaves), kMaxBlocks);
    for (int32_t s0 = 0; s0 < steps; s0 += kJointSteps) {        // a row's arithmetic is the same sequence however the steps are cut
        const int n = std::min<int32_t>(steps - s0, kJointSteps);
        joint_kernel<<<grid, 64 * kWaves, 0, oea::as_stream(stream)>>>(ent, ent_acc, ent_ce, ent_ce_acc, row_count, n_ent, ld, dim, ent_l2_norm,
                                                                       opt_kind == OEA_OPT_ADAGRAD, lr, n, loss_accum + s0);
        OEA_CHECK_HIP(hipGetLastError());
    }
    return OEA_OK;
}

}  // extern "C"
