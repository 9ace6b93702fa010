// proje_step.hip -- the training step of ProjE (models/neural/proje.py:36-74 of the reference): a log-uniform candidate sampler and a
// sampled-softmax (NCE) step with two batch normalisations under TF's dense Adam.
//
//   H = l2n(ent)[h], Rr = l2n(rel)[r];  BN(X) = (X - mean_b X) / sqrt(var_b X + 1e-3) + beta (biased variance, no scale)
//   out = (BN_in(H) + BN_in(Rr)) o mlp_w + mlp_bias;  X = BN_out(out)
//   true_b = X_b . W[t_b] + b[t_b] - log Q(t_b);  samp_bj = X_b . W[s_j] + b[s_j] - log Q(s_j)
//   loss = sum_b [softplus(-true_b) + sum_j softplus(samp_bj)]
//
// The B x S logit matrix never exists in memory.  Two sweeps of one kernel on v_mfma_f32_32x32x2_f32 (exact fp32 products) recompute
// it tile by tile: a workgroup keeps 32 "fixed" rows in LDS, streams 32-row tiles of the other operand past them, forms the 32 x 32
// logits F G^T, turns them into sigma(.) in LDS and adds sigma G into its 32 x d accumulators.
//   sweep A: fixed = batch rows X, streamed = candidate rows W[s_j]:  dX_b   = sum_j sigma_bj W[s_j]   (+ the loss)
//   sweep B: fixed = candidate rows, streamed = batch rows:          dW[s_j] = sum_b sigma_bj X_b,  db[s_j] = sum_b sigma_bj
// The streamed axis is split over blockIdx.y; every split writes its own partial tile and a second kernel adds the splits in
// split order: no float atomics, a fixed summation order.  Both sweeps work with sigma_bj - sigma(a_j), a_j = b[s_j] - log Q(s_j), the
// part of sigma that depends on the row, about 2 % of it.  In dX the rest, sum_j sigma(a_j) W[s_j], is the same vector in every row:
// the output batch norm's backward removes it exactly, and carried along in fp32 its rounding would come out of the two batch norms
// as the noise floor of the entity and relation gradients; it is summed once in fp64 for the output beta.  In dW[s_j] the rest is
// sigma(a_j) sum_b X_b = sigma(a_j) B beta_out in closed form, added in fp64 when the splits are reduced.  The K tail (d odd, d = 75 in ld = 76) is zero padding of the staged
// operands.  Everything reduced over the batch (the BN statistics and their backward sums, the d-vector gradients) goes through
// per-block fp64 partials summed in block order.  Rows that repeat (hub heads, relations, repeated labels, a label that is also a
// candidate) are summed in the step scratch's element type: fp32 atomics, or int64 fixed point in the deterministic build.
#include "nce_half.h"

namespace {

// ---- workspace ---------------------------------------------------------------------------------------------------------------
struct Layout {
    size_t g_ent, g_rel, g_w, g_b, g_vec;           // dense fp32 gradients (what Adam reads)
    size_t s_ent, s_rel, s_w, s_b;                  // the same rows in the scratch's element type
    size_t last_h, last_r, last_t, last_s, last_n;  // what the previous gradient phase touched
    size_t hn, rn, out, x, dxlab, dx, invh, invr, dtrue;
    size_t p, pc, sums;                             // fp64 block partials [nblk, 4, 128] (pc: candidate tiles); sums [5 stages, 4, 128]
    size_t pa, pb, rowsum, loss_a, loss_l;
    size_t total;
    int nbt, nct, split_a, split_b;
};


static Layout make_layout(int64_t n_ent, int64_t n_rel, int ld, int64_t max_pos, int64_t max_s) {
    Layout L;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += oea::align256(bytes); return at; };
    const size_t E = (size_t)n_ent, R = (size_t)n_rel, B = (size_t)max_pos, S = (size_t)max_s;
    L.g_ent = take(4 * E * ld); L.g_rel = take(4 * R * ld); L.g_w = take(4 * E * ld); L.g_b = take(4 * E); L.g_vec = take(4 * 4 * LP);
    L.s_ent = take(sizeof(grad_t) * E * ld); L.s_rel = take(sizeof(grad_t) * R * ld); L.s_w = take(sizeof(grad_t) * E * ld);
    L.s_b = take(sizeof(grad_t) * E);
    L.last_h = take(4 * B); L.last_r = take(4 * B); L.last_t = take(4 * B); L.last_s = take(4 * S); L.last_n = take(16);
    L.nbt = (int)((B + 31) / 32); L.nct = (int)((S + 31) / 32);
    if (L.nbt < 1) L.nbt = 1;
    if (L.nct < 1) L.nct = 1;
    L.split_a = split_of(L.nbt, L.nct); L.split_b = split_of(L.nct, L.nbt);
    const size_t Bp = (size_t)L.nbt * 32;
    // a smaller batch than the capacity may be split further: split(n) n <= min(kMaxSplit n, kTargetWgs - 1 + n), monotone in n
    const size_t Ba = 32 * std::min<size_t>((size_t)kMaxSplit * L.nbt, (size_t)kTargetWgs - 1 + L.nbt);
    const size_t Sb = 32 * std::min<size_t>((size_t)kMaxSplit * L.nct, (size_t)kTargetWgs - 1 + L.nct);
    L.hn = take(4 * Bp * LP); L.rn = take(4 * Bp * LP); L.out = take(4 * Bp * LP); L.x = take(4 * Bp * LP);
    L.dxlab = take(4 * Bp * LP); L.dx = take(4 * Bp * LP); L.invh = take(4 * Bp); L.invr = take(4 * Bp); L.dtrue = take(4 * Bp);
    L.p = take(8 * (size_t)L.nbt * 4 * LP); L.pc = take(8 * (size_t)L.nct * 4 * LP); L.sums = take(8 * 5 * 4 * LP);
    L.pa = take(4 * Ba * LP); L.pb = take(4 * Sb * LP); L.rowsum = take(4 * Sb);
    L.loss_a = take(8 * Ba / 32); L.loss_l = take(8 * (B / 4 + 1));
    L.total = o;
    return L;
}


// ---- clearing what the previous gradient phase touched --------------------------------------------------------------------------

// ---- projection forward ----------------------------------------------------------------------------------------------------------
// one wave per batch row: the two normalised rows into the batch buffers (all LP columns written, zero from dim on), the ids
// into the saved lists
__global__ __launch_bounds__(256) void gather_kernel(Bufs W, const float *__restrict__ ent, const float *__restrict__ rel, int ld, int dim,
                                                     const int32_t *__restrict__ pos, int n_pos, const int32_t *__restrict__ sampled,
                                                     int n_s) {
    const int lane = threadIdx.x & 63;
    const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (int64_t)gridDim.x * 4;
    for (int64_t b = gw; b < n_pos; b += nw) {
        const int32_t h = pos[3 * b], r = pos[3 * b + 1], t = pos[3 * b + 2];
        const float2 a = load2(ent + (int64_t)h * ld, dim, lane), u = load2(rel + (int64_t)r * ld, dim, lane);
        const float ia = rsqrtf(fmaxf(dot2(a, a), 1e-12f)), iu = rsqrtf(fmaxf(dot2(u, u), 1e-12f));
        *reinterpret_cast<float2 *>(W.hn + b * LP + 2 * lane) = make_float2(a.x * ia, a.y * ia);
        *reinterpret_cast<float2 *>(W.rn + b * LP + 2 * lane) = make_float2(u.x * iu, u.y * iu);
        if (lane == 0) {
            W.invh[b] = ia; W.invr[b] = iu;
            W.last_h[b] = h; W.last_r[b] = r; W.last_t[b] = t;
        }
    }
    for (int64_t j = gw * 64 + lane; j < n_s; j += nw * 64) W.last_s[j] = sampled[j];
    if (blockIdx.x == 0 && threadIdx.x == 0) { W.last_n[0] = n_pos; W.last_n[1] = n_s; }
}


// thread = column, block = kRows batch rows; stage 1: sum / sum of squares of Hn and Rn
__global__ __launch_bounds__(LP) void stats1_kernel(Bufs W, int n_pos) {
    const int c = threadIdx.x;
    const int b0 = blockIdx.x * kRows, b1 = min(b0 + kRows, n_pos);
    double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    for (int b = b0; b < b1; ++b) {
        const double h = W.hn[(size_t)b * LP + c], r = W.rn[(size_t)b * LP + c];
        s0 += h; s1 += h * h; s2 += r; s3 += r * r;
    }
    double *p = W.p + (size_t)blockIdx.x * 4 * LP + c;
    p[0] = s0; p[LP] = s1; p[2 * LP] = s2; p[3 * LP] = s3;
}

// stage 2: out = ((Hn - mH) isH + (Rn - mR) isR + 2 beta_in) w + bias; sum / sum of squares of out
__global__ __launch_bounds__(LP) void out_kernel(Bufs W, int n_pos, int dim, const float *__restrict__ beta_in,
                                                 const float *__restrict__ mlp_w, const float *__restrict__ mlp_b) {
    const int c = threadIdx.x;
    const int b0 = blockIdx.x * kRows, b1 = min(b0 + kRows, n_pos);
    const double inv_n = 1.0 / (double)n_pos;
    const double *S = W.sums;
    const Stat sh = stat_of(S[c], S[LP + c], inv_n), sr = stat_of(S[2 * LP + c], S[3 * LP + c], inv_n);
    const bool on = c < dim;
    const float be = on ? beta_in[c] : 0.f, w = on ? mlp_w[c] : 0.f, bi = on ? mlp_b[c] : 0.f;
    double s0 = 0, s1 = 0;
    for (int b = b0; b < b1; ++b) {
        const float ah = (W.hn[(size_t)b * LP + c] - sh.mean) * sh.istd, ch = (W.rn[(size_t)b * LP + c] - sr.mean) * sr.istd;
        const float o = on ? ((ah + be) + (ch + be)) * w + bi : 0.f;
        W.out[(size_t)b * LP + c] = o;
        s0 += (double)o; s1 += (double)o * (double)o;
    }
    double *p = W.p + (size_t)blockIdx.x * 4 * LP + c;
    p[0] = s0; p[LP] = s1;
}



// ---- projection backward ---------------------------------------------------------------------------------------------------------
// stage 4: dX' = dX - c (the row-dependent part) = label part + the splits of sweep A in split order; sums of dX' and dX' o xhat
// (the batch norm's backward of dX' is that of dX)
__global__ __launch_bounds__(LP) void dx_kernel(Bufs W, int n_pos, int dim, int rows_p, int n_split) {
    const int c = threadIdx.x;
    const int b0 = blockIdx.x * kRows, b1 = min(b0 + kRows, n_pos);
    const double inv_n = 1.0 / (double)n_pos;
    const double *S = W.sums + 4 * LP;
    const Stat so = stat_of(S[c], S[LP + c], inv_n);
    double s0 = 0, s1 = 0;
    for (int b = b0; b < b1; ++b) {
        double gd = (double)W.dxlab[(size_t)b * LP + c];
        for (int k = 0; k < n_split; ++k) gd += (double)W.pa[((size_t)k * rows_p + b) * LP + c];
        const float g = c < dim ? (float)gd : 0.f;
        W.dx[(size_t)b * LP + c] = g;
        const float xh = (W.out[(size_t)b * LP + c] - so.mean) * so.istd;
        s0 += (double)g; s1 += (double)g * (double)xh;
    }
    double *p = W.p + (size_t)blockIdx.x * 4 * LP + c;
    p[0] = s0; p[LP] = s1;
}

// stage 5: dout = isO (dX - mean dX - xhat mean(dX xhat)) over dX in place; sums of dout, dout o Ahat, dout o Chat
__global__ __launch_bounds__(LP) void dout_kernel(Bufs W, int n_pos, int dim) {
    const int c = threadIdx.x;
    const int b0 = blockIdx.x * kRows, b1 = min(b0 + kRows, n_pos);
    const double inv_n = 1.0 / (double)n_pos;
    const double *S1 = W.sums, *S2 = W.sums + 4 * LP, *S3 = W.sums + 8 * LP;
    const Stat sh = stat_of(S1[c], S1[LP + c], inv_n), sr = stat_of(S1[2 * LP + c], S1[3 * LP + c], inv_n);
    const Stat so = stat_of(S2[c], S2[LP + c], inv_n);
    const float m0 = (float)(S3[c] * inv_n), m1 = (float)(S3[LP + c] * inv_n);
    double s0 = 0, s1 = 0, s2 = 0;
    for (int b = b0; b < b1; ++b) {
        const size_t at = (size_t)b * LP + c;
        const float xh = (W.out[at] - so.mean) * so.istd;
        const float d = c < dim ? so.istd * (W.dx[at] - m0 - xh * m1) : 0.f;
        W.dx[at] = d;
        const float ah = (W.hn[at] - sh.mean) * sh.istd, ch = (W.rn[at] - sr.mean) * sr.istd;
        s0 += (double)d; s1 += (double)d * (double)ah; s2 += (double)d * (double)ch;
    }
    double *p = W.p + (size_t)blockIdx.x * 4 * LP + c;
    p[0] = s0; p[LP] = s1; p[2 * LP] = s2;
}

// stage 6, one wave per batch row: through BN_in and the row normalisation into the scratch rows of ent[h] and rel[r]; block 0
// also writes the four d-vector gradients
__global__ __launch_bounds__(256) void rows_kernel(Bufs W, int n_pos, int dim, int ld, const float *__restrict__ beta_in,
                                                   const float *__restrict__ mlp_w, const int32_t *__restrict__ pos) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double inv_n = 1.0 / (double)n_pos;
    const double *S1 = W.sums, *S3 = W.sums + 8 * LP, *S4 = W.sums + 12 * LP, *SC = W.sums + 16 * LP;
    if (blockIdx.x == 0 && threadIdx.x < LP) {
        const int c = threadIdx.x;
        const bool on = c < dim;
        const float w = on ? mlp_w[c] : 0.f, be = on ? beta_in[c] : 0.f;
        const double d0 = S4[c];
        W.g_vec[c] = on ? (float)(2.0 * (double)w * d0) : 0.f;                                          // input beta
        W.g_vec[LP + c] = on ? (float)(S4[LP + c] + S4[2 * LP + c] + 2.0 * (double)be * d0) : 0.f;      // mlp_w
        W.g_vec[2 * LP + c] = on ? (float)d0 : 0.f;                                                     // mlp_bias
        W.g_vec[3 * LP + c] = on ? (float)(S3[c] + (double)n_pos * SC[c]) : 0.f;                        // output beta: the common part back
    }
    const int b = blockIdx.x * 4 + wave;
    if (b >= n_pos) return;
    const int c = 2 * lane;
    const float2 d = *reinterpret_cast<const float2 *>(W.dx + (size_t)b * LP + c);
    float2 w = make_float2(0.f, 0.f);
    if (c < dim) w.x = mlp_w[c];
    if (c + 1 < dim) w.y = mlp_w[c + 1];
    const float2 da = make_float2(d.x * w.x, d.y * w.y);
    const float mda0 = (float)(S4[c] * inv_n) * w.x, mda1 = (float)(S4[c + 1] * inv_n) * w.y;
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const double *Ss = S1 + 2 * side * LP, *Sd = S4 + (1 + side) * LP;
        const Stat t0 = stat_of(Ss[c], Ss[LP + c], inv_n), t1 = stat_of(Ss[c + 1], Ss[LP + c + 1], inv_n);
        const float2 u = *reinterpret_cast<const float2 *>((side ? W.rn : W.hn) + (size_t)b * LP + c);
        const float xh0 = (u.x - t0.mean) * t0.istd, xh1 = (u.y - t1.mean) * t1.istd;
        float2 g;                                   // gradient w.r.t. the normalised row
        g.x = c < dim ? t0.istd * (da.x - mda0 - xh0 * ((float)(Sd[c] * inv_n) * w.x)) : 0.f;
        g.y = c + 1 < dim ? t1.istd * (da.y - mda1 - xh1 * ((float)(Sd[c + 1] * inv_n) * w.y)) : 0.f;
        const float pr = dot2(u, g), inv = side ? W.invr[b] : W.invh[b];
        const int64_t row = pos[3 * b + side];
        grad_t *dst = (side ? W.s_rel : W.s_ent) + row * ld;
        if (c < dim) oea::grad_add(dst + c, (g.x - u.x * pr) * inv);
        if (c + 1 < dim) oea::grad_add(dst + c + 1, (g.y - u.y * pr) * inv);
    }
}


static Bufs bufs_of(void *ws, const Layout &L) {
    char *b = static_cast<char *>(ws);
    Bufs W;
    W.g_ent = (float *)(b + L.g_ent); W.g_rel = (float *)(b + L.g_rel); W.g_w = (float *)(b + L.g_w); W.g_b = (float *)(b + L.g_b);
    W.g_vec = (float *)(b + L.g_vec);
    W.s_ent = (grad_t *)(b + L.s_ent); W.s_rel = (grad_t *)(b + L.s_rel); W.s_w = (grad_t *)(b + L.s_w); W.s_b = (grad_t *)(b + L.s_b);
    W.last_h = (int32_t *)(b + L.last_h); W.last_r = (int32_t *)(b + L.last_r); W.last_t = (int32_t *)(b + L.last_t);
    W.last_s = (int32_t *)(b + L.last_s); W.last_n = (int32_t *)(b + L.last_n);
    W.hn = (float *)(b + L.hn); W.rn = (float *)(b + L.rn); W.out = (float *)(b + L.out); W.x = (float *)(b + L.x);
    W.dxlab = (float *)(b + L.dxlab); W.dx = (float *)(b + L.dx); W.invh = (float *)(b + L.invh); W.invr = (float *)(b + L.invr);
    W.dtrue = (float *)(b + L.dtrue);
    W.p = (double *)(b + L.p); W.pc = (double *)(b + L.pc); W.sums = (double *)(b + L.sums);
    W.pa = (float *)(b + L.pa); W.pb = (float *)(b + L.pb); W.rowsum = (float *)(b + L.rowsum);
    W.loss_a = (double *)(b + L.loss_a); W.loss_l = (double *)(b + L.loss_l);
    return W;
}

static int check_shape(const char *who, int64_t n_ent, int64_t n_rel, int32_t dim, int32_t ld, int64_t max_pos, int64_t max_s) {
    if (!(n_ent > 0 && n_rel > 0 && max_pos >= 0 && max_s >= 0 && n_ent < (1LL << 31) && max_pos < (1LL << 24) && max_s < (1LL << 24))) {
        oea::set_error("%s: invalid argument: table rows / batch capacity", who);
        return OEA_EINVAL;
    }
    if (!(ld % 4 == 0)) { oea::set_error("%s: invalid argument: ld %% 4 == 0", who); return OEA_EINVAL; }
    if (!(dim > 0 && dim <= ld)) { oea::set_error("%s: invalid argument: 0 < dim <= ld", who); return OEA_EINVAL; }
    if (dim > kMaxDim) { oea::set_error("%s: dim %d > %d", who, dim, kMaxDim); return OEA_EUNSUPPORTED; }
    return OEA_OK;
}

}  // namespace

extern "C" {

size_t oea_proje_workspace_floats(int64_t n_ent, int64_t n_rel, int32_t dim, int32_t ld, int64_t max_pos, int64_t max_sampled) {
    if (check_shape("oea_proje_workspace_floats", n_ent, n_rel, dim, ld, max_pos, max_sampled) != OEA_OK) return 0;
    return make_layout(n_ent, n_rel, ld, max_pos, max_sampled).total / 4;
}

int oea_proje_grads(void *workspace, int64_t n_ent, int64_t n_rel, int32_t dim, int32_t ld, int64_t max_pos, int64_t max_sampled,
                    void **grads) {
    const int rc = check_shape("oea_proje_grads", n_ent, n_rel, dim, ld, max_pos, max_sampled);
    if (rc != OEA_OK) return rc;
    OEA_REQUIRE(workspace && grads, "null pointer");
    const Layout L = make_layout(n_ent, n_rel, ld, max_pos, max_sampled);
    const Bufs W = bufs_of(workspace, L);
    grads[0] = W.g_ent; grads[1] = W.g_rel; grads[2] = W.g_w; grads[3] = W.g_b;
    for (int i = 0; i < 4; ++i) grads[4 + i] = W.g_vec + i * LP;
    return OEA_OK;
}

int oea_proje_step(const oea_proje_vars *vars, int64_t n_ent, int64_t n_rel, int32_t dim, int32_t ld, const int32_t *pos, int64_t n_pos,
                   const int32_t *sampled, const float *log_q_sampled, int64_t n_sampled, const int64_t *num_tries, int64_t t, float lr,
                   void *workspace, int64_t max_pos, int64_t max_sampled, double *loss_accum, int32_t phase, void *stream) {
    OEA_REQUIRE(vars && workspace && loss_accum, "null pointer");
    for (int i = 0; i < 8; ++i) OEA_REQUIRE(vars->p[i] && vars->m[i] && vars->v[i], "null variable / moment");
    OEA_REQUIRE(phase == OEA_PHASE_BOTH || phase == OEA_PHASE_GRAD || phase == OEA_PHASE_APPLY, "phase");
    const int rc = check_shape("oea_proje_step", n_ent, n_rel, dim, ld, max_pos, max_sampled);
    if (rc != OEA_OK) return rc;
    OEA_REQUIRE(n_pos >= 1 && n_pos <= max_pos && pos, "1 <= n_pos <= max_pos");
    OEA_REQUIRE(n_sampled >= 2 && n_sampled <= max_sampled && n_sampled <= n_ent, "2 <= n_sampled <= min(max_sampled, n_ent)");
    OEA_REQUIRE(sampled && log_q_sampled && num_tries, "sampled / log_q_sampled / num_tries");
    OEA_REQUIRE(t >= 1, "t >= 1");
    hipStream_t st = oea::as_stream(stream);
    const Layout L = make_layout(n_ent, n_rel, ld, max_pos, max_sampled);
    const Bufs W = bufs_of(workspace, L);
    const int B = (int)n_pos, S = (int)n_sampled;
    const int nbt = (B + 31) / 32, nct = (S + 31) / 32, nwb = (B + 3) / 4;
    const float *ent = vars->p[0], *rel = vars->p[1], *ent_w = vars->p[2], *ent_b = vars->p[3];
    const float *beta_in = vars->p[4], *mlp_w = vars->p[5], *mlp_b = vars->p[6], *beta_out = vars->p[7];
    if (phase != OEA_PHASE_APPLY) {
        const int split_a = split_of(nbt, nct), split_b = split_of(nct, nbt);       // <= the layout's: it is sized for the capacities
        const int nt = (dim + 31) / 32;
        const int64_t cap = std::max(max_pos, max_sampled);
        clear_prev_kernel<<<(unsigned)std::min<int64_t>(oea::ceil_div(cap, 4), 4096), 256, 0, st>>>(W, ld, cap);
        gather_kernel<<<(unsigned)std::min<int64_t>(oea::ceil_div(std::max(B, (S + 63) / 64), 4), 4096), 256, 0, st>>>(W, ent, rel, ld, dim, pos,
                                                                                                                      B, sampled, S);
        stats1_kernel<<<nbt, LP, 0, st>>>(W, B);
        finalize_kernel<<<1, LP * kChains, 0, st>>>(W.p, nbt, 4, W.sums);
        out_kernel<<<nbt, LP, 0, st>>>(W, B, dim, beta_in, mlp_w, mlp_b);
        finalize_kernel<<<1, LP * kChains, 0, st>>>(W.p, nbt, 2, W.sums + 4 * LP);
        label_kernel<true><<<nwb, 256, 0, st>>>(W, B, dim, ld, beta_out, ent_w, ent_b, pos, num_tries, 1.0 / log((double)n_ent + 1.0));
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
        reduce_cand_kernel<true><<<S, LP, 0, st>>>(W, sampled, log_q_sampled, ent_b, beta_out, nullptr, B, S, nct * 32, split_b, dim, ld);
        dx_kernel<<<nbt, LP, 0, st>>>(W, B, dim, nbt * 32, split_a);
        finalize_kernel<<<1, LP * kChains, 0, st>>>(W.p, nbt, 2, W.sums + 8 * LP);
        dout_kernel<<<nbt, LP, 0, st>>>(W, B, dim);
        finalize_kernel<<<1, LP * kChains, 0, st>>>(W.p, nbt, 3, W.sums + 12 * LP);
        rows_kernel<<<nwb, 256, 0, st>>>(W, B, dim, ld, beta_in, mlp_w, pos);
        convert_kernel<<<(unsigned)std::min<int64_t>(oea::ceil_div(std::max(B, S), 4), 4096), 256, 0, st>>>(W, ld, B, S);
        loss_kernel<<<1, 64, 0, st>>>(W.loss_l, nwb, W.loss_a, nbt * split_a, loss_accum);
        OEA_CHECK_HIP(hipGetLastError());
    }
    if (phase != OEA_PHASE_GRAD) {
        const float *g[8] = {W.g_ent, W.g_rel, W.g_w, W.g_b, W.g_vec, W.g_vec + LP, W.g_vec + 2 * LP, W.g_vec + 3 * LP};
        const int64_t n[8] = {n_ent * ld, n_rel * ld, n_ent * ld, n_ent, dim, dim, dim, dim};
        for (int i = 0; i < 8; ++i) {
            const int r = oea_adam_dense(vars->p[i], g[i], vars->m[i], vars->v[i], n[i], lr, 0.9f, 0.999f, 1e-8f, t, stream);
            if (r != OEA_OK) return r;
        }
    }
    return OEA_OK;
}

}  // extern "C"
