// row_ops.h -- the helpers of every kernel that gives a wave one row (semantic_step.hip, jape_step.hip, attr2vec_step.hip, nce_half.h):
// a lane holds columns 2 l and 2 l + 1 of a row of up to 128 columns; the logistic pair and log Q of the sampled softmax
// (log_uniform.hip draws under it); gradient rows that leave the wave through the step engine's scratch.
#pragma once
#include "common.h"

namespace oea {
namespace row {

// columns 2 lane, 2 lane + 1 of a row (zero from dim on); ld % 4 == 0 keeps the float2 inside the row
__device__ __forceinline__ float2 load2(const float *row, int dim, int lane) {
    const int c = 2 * lane;
    float2 v = make_float2(0.f, 0.f);
    if (c < dim) {
        v = *reinterpret_cast<const float2 *>(row + c);
        if (c + 1 >= dim) v.y = 0.f;
    }
    return v;
}
__device__ __forceinline__ float dot2(float2 a, float2 b) { return oea::group_sum<64>(fmaf(a.x, b.x, a.y * b.y)); }
__device__ __forceinline__ float inv_norm(float2 a, int on) { return on ? rsqrtf(fmaxf(dot2(a, a), 1e-12f)) : 1.f; }
__device__ __forceinline__ float2 scale2(float2 a, float s) { return make_float2(a.x * s, a.y * s); }
__device__ __forceinline__ float2 mul2(float2 a, float2 b) { return make_float2(a.x * b.x, a.y * b.y); }
__device__ __forceinline__ float2 add2(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }

__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float softplus_f(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// log Q of class c after n tries: Q = -expm1(n log1p(-P)), P = (log(c + 2) - log(c + 1)) / log(E + 1)
__device__ __forceinline__ double log_q(int64_t c, double n_tries, double inv_log_e1) {
    const double p = (log((double)(c + 2)) - log((double)(c + 1))) * inv_log_e1;
    return log(-expm1(n_tries * log1p(-p)));
}

// one gradient row into the scratch: the lane pairs go through the wave's LDS row so that each atomic instruction covers 64
// contiguous floats (columns lane and lane + 64)
__device__ __forceinline__ void flush_row(grad_t *grad, flag_t *touched, int64_t row, float2 g, int ld, int dim, int lane,
                                          float *buf) {
    __builtin_amdgcn_wave_barrier();
    *reinterpret_cast<float2 *>(buf + 2 * lane) = g;
    __builtin_amdgcn_wave_barrier();
    grad_t *p = grad + row * ld;
    if (lane < dim) oea::grad_add(p + lane, buf[lane]);
    if (lane + 64 < dim) oea::grad_add(p + lane + 64, buf[lane + 64]);
    if (lane == 0) touched[row] = 1;
}

// gradient rows of the positive's own rows, summed in registers; a row of a negative that matches one of them is added
// there (the first match: duplicate ids in the positive share the first slot), any other row goes out at once
template <int NS>
struct Slots {
    int64_t id[NS];
    float2 g[NS];
    __device__ __forceinline__ void set(int i, int64_t row) { id[i] = row; g[i] = make_float2(0.f, 0.f); }
    __device__ __forceinline__ void add(int64_t row, float2 v, grad_t *grad, flag_t *touched, int ld, int dim, int lane, float *buf) {
        bool done = false;
#pragma unroll
        for (int i = 0; i < NS; ++i) {       // selects, not a branch: a branch lets the compiler index g[] (scratch)
            const bool hit = !done && id[i] == row;
            g[i] = add2(g[i], hit ? v : make_float2(0.f, 0.f));
            done |= hit;
        }
        if (!done) flush_row(grad, touched, row, v, ld, dim, lane, buf);
    }
    __device__ __forceinline__ void flush(grad_t *grad, flag_t *touched, int ld, int dim, int lane, float *buf) {
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            bool dup = false;
#pragma unroll
            for (int j = 0; j < i; ++j) dup |= id[j] == id[i];
            if (!dup) flush_row(grad, touched, id[i], g[i], ld, dim, lane, buf);
        }
    }
};

}  // namespace row
}  // namespace oea
