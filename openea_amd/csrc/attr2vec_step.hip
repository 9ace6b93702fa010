// attr2vec_step.hip -- JAPE's attribute embedding (approaches/attr2vec.py:106-124 of the reference): a skip-gram over co-occurring
// attribute pairs under tf.nn.nce_loss and Adagrad, both tables seen through the row normalisation (xavier_init(..., True)).
//
//   x_b = l2n(embeds)[in_b], w_c = l2n(nce_weights)[c], a_j = bias[s_j] - log Q(s_j)
//   true_b = x_b . w_lab + bias[lab] - log Q(lab);  samp_bj = x_b . w_sj + a_j
//   loss = mean_b ( softplus(-true_b) + sum_j softplus(samp_bj) )
//
// A is 700 to 1,400 on the benchmark datasets while the batch holds 5,000 to 20,000 pairs, and the sampled half of a row depends
// on its INPUT id alone.  So the batch is reduced first: n[a] = the multiplicity of input a (integer atomics), and the sampled half
// runs over distinct inputs x candidates with the weight n[a] / B -- an A x S x d problem instead of B x S x d.
//   true_kernel    one wave per pair: the true logit, its two gradient rows and the bias entry into the scratch, n[in] += 1
//   cand_kernel    one wave per candidate: l2n(W[s_j]) row-major (WN) and transposed (WNT), a_j
//   samp_kernel    one wave per input a with n[a] > 0, a lane per candidate: G[a, j] = (n[a] / B) sigmoid(samp_aj) from WNT, then
//                  dL/dx_a = sum_j G[a, j] WN[j] with a lane per column pair
//   gradw_kernel   one wave per candidate: dL/dw_sj = sum_a G[a, j] x_a, dL/db_sj = sum_a G[a, j], in ascending a
//   finish_kernel  one wave per table row: the scratch sums back through the row normalisation into the dense fp32 gradients
//                  (zero rows where the batch touched nothing); leaves scratch, counts and flags zeroed for the next step
//   apply_kernel   one wave per table row with a flag: Adagrad, acc += g^2, v -= lr g / sqrt(acc); other rows keep their bits
// Rows that repeat (an input in many pairs, a repeated label, a label that is also a candidate) are summed in the step scratch's
// element type: fp32 atomics, or int64 fixed point in the deterministic build, where every other sum above has a fixed order.
//
// The candidates come from log_uniform.hip; oea_attr2vec_epoch takes those of all its steps from oea_log_uniform_sample_steps, whose
// status word per step the kernels here read.
#include "row_ops.h"

#include <algorithm>

namespace {

using oea::grad_t;
using namespace oea::row;

constexpr int kMaxDim = 128;
constexpr int LP = 128;            // row stride of xn / wn (zero padded)

// ---- workspace -------------------------------------------------------------------------------------------------------------
struct A2V {
    float *g_emb, *g_w, *g_b;              // dense fp32 gradients w.r.t. the variables
    grad_t *s_x, *s_w, *s_b;               // sums w.r.t. the normalised rows and the bias
    int32_t *cnt, *tx, *tw, *ax, *aw;      // multiplicity of an input; touched this step (x / w rows); to be applied
    float *xn, *wn, *wnt, *aj, *G;
    int64_t sp;                            // candidate stride of wnt and G
    size_t total;
};

static A2V make_a2v(void *base, int64_t n_attr, int ld, int64_t max_s) {
    A2V L;
    size_t o = 0;
    char *b = static_cast<char *>(base);
    auto take = [&](size_t bytes) { char *at = b + o; o += oea::align256(bytes); return at; };
    const size_t A = (size_t)n_attr, Sp = ((size_t)max_s + 63) / 64 * 64;
    L.sp = (int64_t)Sp;
    L.g_emb = (float *)take(4 * A * ld); L.g_w = (float *)take(4 * A * ld); L.g_b = (float *)take(4 * A);
    L.s_x = (grad_t *)take(sizeof(grad_t) * A * ld); L.s_w = (grad_t *)take(sizeof(grad_t) * A * ld); L.s_b = (grad_t *)take(sizeof(grad_t) * A);
    L.cnt = (int32_t *)take(4 * A); L.tx = (int32_t *)take(4 * A); L.tw = (int32_t *)take(4 * A);
    L.ax = (int32_t *)take(4 * A); L.aw = (int32_t *)take(4 * A);
    L.xn = (float *)take(4 * A * LP); L.wn = (float *)take(4 * Sp * LP); L.wnt = (float *)take(4 * LP * Sp); L.aj = (float *)take(4 * Sp);
    L.G = (float *)take(4 * A * Sp);
    L.total = o;
    return L;
}

struct StepArgs {
    A2V W;
    const float *emb, *wts, *bias;
    int ld, dim;
    int64_t n_attr;
    const int32_t *pairs, *idx;            // pair b = pairs[idx ? idx[b] : b]
    int64_t n_batch;
    const int32_t *sampled;
    const float *logq;
    const int64_t *num_tries;
    int n_s;
    const int32_t *status;         // the sampler's word for this step (NULL: none): != 0 and the step does nothing
    double *loss_accum;
};

__device__ __forceinline__ void add_row(grad_t *p, float2 g, int dim, int lane) {
    const int c = 2 * lane;
    if (c < dim) oea::grad_add(p + c, g.x);
    if (c + 1 < dim) oea::grad_add(p + c + 1, g.y);
}

__global__ __launch_bounds__(256) void true_kernel(StepArgs A) {
    if (A.status && *A.status != 0) return;        // grid-uniform
    const int lane = threadIdx.x & 63;
    const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (int64_t)gridDim.x * 4;
    const double n_tries = (double)*A.num_tries, inv_log = 1.0 / log((double)A.n_attr + 1.0);
    const float inv_b = 1.f / (float)A.n_batch;
    double loss_local = 0.0;
    for (int64_t b = gw; b < A.n_batch; b += nw) {
        const int64_t at = A.idx ? A.idx[b] : b;
        const int32_t in = A.pairs[2 * at], lab = A.pairs[2 * at + 1];
        const float2 a = load2(A.emb + (int64_t)in * A.ld, A.dim, lane), u = load2(A.wts + (int64_t)lab * A.ld, A.dim, lane);
        const float ia = rsqrtf(fmaxf(dot2(a, a), 1e-12f)), iu = rsqrtf(fmaxf(dot2(u, u), 1e-12f));
        const float2 x = make_float2(a.x * ia, a.y * ia), w = make_float2(u.x * iu, u.y * iu);
        const float logit = dot2(x, w) + A.bias[lab] - (float)log_q(lab, n_tries, inv_log);
        loss_local += (double)(softplus_f(-logit) * inv_b);
        const float dl = -sigmoid_f(-logit) * inv_b;
        add_row(A.W.s_x + (int64_t)in * A.ld, make_float2(dl * w.x, dl * w.y), A.dim, lane);
        add_row(A.W.s_w + (int64_t)lab * A.ld, make_float2(dl * x.x, dl * x.y), A.dim, lane);
        if (lane == 0) {
            oea::grad_add(A.W.s_b + lab, dl);
            atomicAdd(A.W.cnt + in, 1);
            A.W.tx[in] = 1; A.W.tw[lab] = 1;
        }
    }
    oea::block_loss_add<4>(loss_local, lane, threadIdx.x >> 6, A.loss_accum);
}

__global__ __launch_bounds__(256) void cand_kernel(StepArgs A) {
    if (A.status && *A.status != 0) return;
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= A.n_s) return;
    const int32_t id = A.sampled[j];
    const float2 u = load2(A.wts + (int64_t)id * A.ld, A.dim, lane);
    const float iu = rsqrtf(fmaxf(dot2(u, u), 1e-12f));
    const float2 w = make_float2(u.x * iu, u.y * iu);
    *reinterpret_cast<float2 *>(A.W.wn + (int64_t)j * LP + 2 * lane) = w;
    A.W.wnt[(int64_t)(2 * lane) * A.W.sp + j] = w.x;
    A.W.wnt[(int64_t)(2 * lane + 1) * A.W.sp + j] = w.y;
    if (lane == 0) A.W.aj[j] = A.bias[id] - A.logq[j];
}

__global__ __launch_bounds__(256) void samp_kernel(StepArgs A) {
    __shared__ __attribute__((aligned(16))) float xs[4][LP];
    __shared__ float gs[4][64];
    if (A.status && *A.status != 0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t gw = (int64_t)blockIdx.x * 4 + wave, nw = (int64_t)gridDim.x * 4;
    const float inv_b = 1.f / (float)A.n_batch;
    const int64_t sp = A.W.sp;
    double loss_local = 0.0;
    for (int64_t a = gw; a < A.n_attr; a += nw) {
        const int n = A.W.cnt[a];
        if (n == 0) continue;                         // wave-uniform
        const float wgt = (float)n * inv_b;
        const float2 v = load2(A.emb + a * A.ld, A.dim, lane);
        const float iv = rsqrtf(fmaxf(dot2(v, v), 1e-12f));
        const float2 x = make_float2(v.x * iv, v.y * iv);
        *reinterpret_cast<float2 *>(A.W.xn + a * LP + 2 * lane) = x;
        __builtin_amdgcn_wave_barrier();
        *reinterpret_cast<float2 *>(xs[wave] + 2 * lane) = x;
        __builtin_amdgcn_wave_barrier();
        float2 gx = make_float2(0.f, 0.f);
        float lsum = 0.f;
        for (int j0 = 0; j0 < A.n_s; j0 += 64) {
            const int j = j0 + lane;
            float sg = 0.f;
            if (j < A.n_s) {
                float acc = 0.f;
                const float *wt = A.W.wnt + j;
                for (int c = 0; c < A.dim; ++c) acc = fmaf(xs[wave][c], wt[(int64_t)c * sp], acc);
                const float logit = acc + A.W.aj[j];
                sg = wgt * sigmoid_f(logit);
                lsum += wgt * softplus_f(logit);
                A.W.G[a * sp + j] = sg;
            }
            gs[wave][lane] = sg;
            __builtin_amdgcn_wave_barrier();
            const int jn = min(64, A.n_s - j0);
            for (int jj = 0; jj < jn; ++jj) {
                const float g = gs[wave][jj];
                const float2 wv = *reinterpret_cast<const float2 *>(A.W.wn + (int64_t)(j0 + jj) * LP + 2 * lane);
                gx.x = fmaf(g, wv.x, gx.x); gx.y = fmaf(g, wv.y, gx.y);
            }
            __builtin_amdgcn_wave_barrier();
        }
        add_row(A.W.s_x + a * A.ld, gx, A.dim, lane);
        loss_local += (double)oea::group_sum<64>(lsum);
    }
    oea::block_loss_add<4>(loss_local, lane, wave, A.loss_accum);
}

__global__ __launch_bounds__(256) void gradw_kernel(StepArgs A) {
    if (A.status && *A.status != 0) return;
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= A.n_s) return;
    float2 acc = make_float2(0.f, 0.f);
    float db = 0.f;
    for (int64_t a = 0; a < A.n_attr; ++a) {
        if (A.W.cnt[a] == 0) continue;
        const float g = A.W.G[a * A.W.sp + j];
        const float2 x = *reinterpret_cast<const float2 *>(A.W.xn + a * LP + 2 * lane);
        acc.x = fmaf(g, x.x, acc.x); acc.y = fmaf(g, x.y, acc.y);
        db += g;
    }
    const int32_t id = A.sampled[j];
    add_row(A.W.s_w + (int64_t)id * A.ld, acc, A.dim, lane);
    if (lane == 0) { oea::grad_add(A.W.s_b + id, db); A.W.tw[id] = 1; }
}

// y = v rsqrt(max(|v|^2, 1e-12)):  dL/dv = inv (g - y (y . g)) above the clamp, inv g below it
__device__ __forceinline__ float2 norm_back(float2 v, float2 g) {
    const float ss = dot2(v, v);
    const float inv = rsqrtf(fmaxf(ss, 1e-12f));
    if (ss < 1e-12f) return make_float2(g.x * inv, g.y * inv);
    const float2 y = make_float2(v.x * inv, v.y * inv);
    const float p = dot2(y, g);
    return make_float2((g.x - y.x * p) * inv, (g.y - y.y * p) * inv);
}

__device__ __forceinline__ void finish_row(const float *table, grad_t *s, float *g, int64_t r, int ld, int dim, int lane, bool on) {
    const int c = 2 * lane;
    float2 out = make_float2(0.f, 0.f);
    if (on) {
        float2 gn = make_float2(0.f, 0.f);
        if (c < dim) { gn.x = oea::grad_val(s[r * ld + c]); s[r * ld + c] = 0; }
        if (c + 1 < dim) { gn.y = oea::grad_val(s[r * ld + c + 1]); s[r * ld + c + 1] = 0; }
        out = norm_back(load2(table + r * ld, dim, lane), gn);
    }
    if (c < ld) *reinterpret_cast<float2 *>(g + r * ld + c) = out;        // ld is even: the pair stays inside the row
}

__global__ __launch_bounds__(256) void finish_kernel(StepArgs A) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= A.n_attr) return;
    const bool on_x = A.W.tx[r] != 0, on_w = A.W.tw[r] != 0;
    finish_row(A.emb, A.W.s_x, A.W.g_emb, r, A.ld, A.dim, lane, on_x);
    finish_row(A.wts, A.W.s_w, A.W.g_w, r, A.ld, A.dim, lane, on_w);
    if (lane == 0) {
        A.W.g_b[r] = on_w ? oea::grad_val(A.W.s_b[r]) : 0.f;
        A.W.s_b[r] = 0;
        A.W.ax[r] = on_x; A.W.aw[r] = on_w;
        A.W.tx[r] = 0; A.W.tw[r] = 0; A.W.cnt[r] = 0;
    }
}

__device__ __forceinline__ void adagrad_row(float *v, float *acc, const float *g, int dim, int lane, float lr) {
    for (int c = lane; c < dim; c += 64) {
        const float gg = g[c], a = acc[c] + gg * gg;
        acc[c] = a;
        v[c] -= lr * gg / sqrtf(a);
    }
}

struct ApplyArgs {
    A2V W;
    float *emb, *emb_acc, *wts, *wts_acc, *bias, *bias_acc;
    int ld, dim;
    int64_t n_attr;
    float lr;
};

__global__ __launch_bounds__(256) void apply_kernel(ApplyArgs A) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= A.n_attr) return;
    if (A.W.ax[r]) adagrad_row(A.emb + r * A.ld, A.emb_acc + r * A.ld, A.W.g_emb + r * A.ld, A.dim, lane, A.lr);
    if (A.W.aw[r]) {
        adagrad_row(A.wts + r * A.ld, A.wts_acc + r * A.ld, A.W.g_w + r * A.ld, A.dim, lane, A.lr);
        if (lane == 0) {
            const float gg = A.W.g_b[r], a = A.bias_acc[r] + gg * gg;
            A.bias_acc[r] = a;
            A.bias[r] -= A.lr * gg / sqrtf(a);
        }
    }
}

int check_a2v(const char *who, const oea_attr2vec_vars *v, int64_t n_attr, int32_t dim, int32_t ld, int64_t n_batch, int64_t n_s,
              int64_t max_s, int32_t phase) {
    OEA_REQUIRE(v && v->embeds && v->nce_weights && v->nce_biases, "null pointer");
    OEA_REQUIRE(phase == OEA_PHASE_GRAD || (v->embeds_acc && v->nce_weights_acc && v->nce_biases_acc), "Adagrad needs its three accumulators");
    OEA_REQUIRE(phase >= OEA_PHASE_BOTH && phase <= OEA_PHASE_APPLY, "phase");
    OEA_REQUIRE(n_attr >= 1 && n_attr < ((int64_t)1 << 31), "1 <= n_attr < 2^31");
    OEA_REQUIRE(ld % 4 == 0, "ld % 4 == 0");
    OEA_REQUIRE(dim > 0 && dim <= ld, "0 < dim <= ld");
    OEA_REQUIRE(max_s >= 1 && max_s < ((int64_t)1 << 24), "1 <= max_sampled < 2^24");
    if (phase != OEA_PHASE_APPLY) {           // the apply phase reads neither the batch nor the candidates
        OEA_REQUIRE(n_batch >= 1 && n_batch < ((int64_t)1 << 31), "1 <= batch < 2^31");
        OEA_REQUIRE(n_s >= 1 && n_s <= max_s && n_s <= n_attr, "1 <= n_sampled <= max_sampled, n_attr");
    }
    if (dim > kMaxDim) {
        oea::set_error("%s: dim %d > %d", who, dim, kMaxDim);
        return OEA_EUNSUPPORTED;
    }
    return OEA_OK;
}

int launch_step(const oea_attr2vec_vars *v, const A2V &W, int64_t n_attr, int dim, int ld, const int32_t *pairs, const int32_t *idx,
                int64_t n_batch, const int32_t *sampled, int n_s, const float *logq, const int64_t *num_tries, const int32_t *status,
                float lr, double *loss_accum, int phase, hipStream_t st) {
    const unsigned row_grid = (unsigned)oea::ceil_div(n_attr, 4);
    if (phase != OEA_PHASE_APPLY) {
        StepArgs A;
        A.W = W; A.emb = v->embeds; A.wts = v->nce_weights; A.bias = v->nce_biases; A.ld = ld; A.dim = dim; A.n_attr = n_attr;
        A.pairs = pairs; A.idx = idx; A.n_batch = n_batch; A.sampled = sampled; A.logq = logq; A.num_tries = num_tries; A.n_s = n_s; A.status = status;
        A.loss_accum = loss_accum;
        true_kernel<<<(unsigned)std::min<int64_t>(oea::ceil_div(n_batch, 4), 4096), 256, 0, st>>>(A);
        cand_kernel<<<(unsigned)oea::ceil_div(n_s, 4), 256, 0, st>>>(A);
        samp_kernel<<<(unsigned)std::min<int64_t>(row_grid, 2048), 256, 0, st>>>(A);
        gradw_kernel<<<(unsigned)oea::ceil_div(n_s, 4), 256, 0, st>>>(A);
        finish_kernel<<<row_grid, 256, 0, st>>>(A);
        OEA_CHECK_HIP(hipGetLastError());
    }
    if (phase != OEA_PHASE_GRAD) {
        ApplyArgs P;
        P.W = W; P.emb = v->embeds; P.emb_acc = v->embeds_acc; P.wts = v->nce_weights; P.wts_acc = v->nce_weights_acc;
        P.bias = v->nce_biases; P.bias_acc = v->nce_biases_acc; P.ld = ld; P.dim = dim; P.n_attr = n_attr; P.lr = lr;
        apply_kernel<<<row_grid, 256, 0, st>>>(P);
        OEA_CHECK_HIP(hipGetLastError());
    }
    return OEA_OK;
}

}  // namespace

extern "C" {

size_t oea_attr2vec_workspace_bytes(int64_t n_attr, int32_t ld, int64_t max_sampled) {
    if (n_attr < 1 || ld < 4 || ld % 4 != 0 || max_sampled < 1 || max_sampled >= ((int64_t)1 << 24)) return 0;
    return make_a2v(nullptr, n_attr, ld, max_sampled).total;
}

int oea_attr2vec_grads(void *workspace, int64_t n_attr, int32_t ld, int64_t max_sampled, void **grads) {
    OEA_REQUIRE(workspace && grads && oea_attr2vec_workspace_bytes(n_attr, ld, max_sampled) != 0, "arguments");
    const A2V W = make_a2v(workspace, n_attr, ld, max_sampled);
    grads[0] = W.g_emb; grads[1] = W.g_w; grads[2] = W.g_b;
    return OEA_OK;
}

int oea_attr2vec_step(const oea_attr2vec_vars *vars, int64_t n_attr, int32_t dim, int32_t ld, const int32_t *pairs, int64_t n_batch,
                      const int32_t *sampled, int64_t n_sampled, const float *log_q_sampled, const int64_t *num_tries, float lr,
                      void *workspace, int64_t max_sampled, double *loss_accum, int32_t phase, void *stream) {
    const int rc = check_a2v("oea_attr2vec_step", vars, n_attr, dim, ld, n_batch, n_sampled, max_sampled, phase);
    if (rc != OEA_OK) return rc;
    OEA_REQUIRE(workspace && loss_accum, "null pointer");
    OEA_REQUIRE(phase == OEA_PHASE_APPLY || (pairs && sampled && log_q_sampled && num_tries), "null pointer");
    return launch_step(vars, make_a2v(workspace, n_attr, ld, max_sampled), n_attr, dim, ld, pairs, nullptr, n_batch, sampled,
                       (int)n_sampled, log_q_sampled, num_tries, nullptr, lr, loss_accum, phase, oea::as_stream(stream));
}

int oea_attr2vec_epoch(const oea_attr2vec_vars *vars, int64_t n_attr, int32_t dim, int32_t ld, const int32_t *pairs, int64_t n_pairs,
                       int64_t n_batch, int32_t steps, uint64_t seed, uint64_t step0, const double *thresholds, int64_t n_sampled,
                       int32_t *cand_ids, int64_t *cand_tries, float *cand_log_q, int32_t *cand_status, int32_t *batch_idx, float lr,
                       void *workspace, int64_t max_sampled, double *loss_accum, void *stream) {
    const int rc = check_a2v("oea_attr2vec_epoch", vars, n_attr, dim, ld, n_batch, n_sampled, max_sampled, OEA_PHASE_BOTH);
    if (rc != OEA_OK) return rc;
    OEA_REQUIRE(steps >= 0, "steps >= 0");
    if (steps == 0) return OEA_OK;            // fewer pairs than one batch: the reference runs no step either (attr2vec.py:186)
    OEA_REQUIRE(workspace && loss_accum && pairs && thresholds && cand_ids && cand_tries && cand_log_q && cand_status && batch_idx,
                "null pointer");
    OEA_REQUIRE(n_pairs >= n_batch && n_pairs < ((int64_t)1 << 31), "batch <= n_pairs < 2^31");
    if (n_attr > OEA_LOG_UNIFORM_STEPS_MAX_CLASSES) {
        oea::set_error("oea_attr2vec_epoch: n_attr %lld > %d (oea_log_uniform_sample_steps)", (long long)n_attr,
                       OEA_LOG_UNIFORM_STEPS_MAX_CLASSES);
        return OEA_EUNSUPPORTED;
    }
    int rs = oea_log_uniform_sample_steps(n_attr, n_sampled, seed, step0, steps, thresholds, cand_ids, cand_tries, cand_log_q,
                                          cand_status, stream);
    if (rs != OEA_OK) return rs;
    const A2V W = make_a2v(workspace, n_attr, ld, max_sampled);
    for (int32_t s = 0; s < steps; ++s) {
        rs = oea_sample_distinct(n_pairs, n_batch, seed, step0 + (uint64_t)s, batch_idx, stream);
        if (rs != OEA_OK) return rs;
        rs = launch_step(vars, W, n_attr, dim, ld, pairs, batch_idx, n_batch, cand_ids + (int64_t)s * n_sampled, (int)n_sampled,
                         cand_log_q + (int64_t)s * n_sampled, cand_tries + s, cand_status + s, lr, loss_accum, OEA_PHASE_BOTH,
                         oea::as_stream(stream));
        if (rs != OEA_OK) return rs;
    }
    return OEA_OK;
}

}  // extern "C"
