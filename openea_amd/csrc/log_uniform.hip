// log_uniform.hip -- the log-uniform candidate sampler of the sampled softmax (tf.nn.log_uniform_candidate_sampler, unique = True),
// for ProjE, ConvE and Attr2Vec.  One draw body, two kernels:
//   oea_log_uniform_sample        one step, one workgroup, any number of classes: the first-appearance table in the workspace; the
//                                 host reads a status word back
//   oea_log_uniform_sample_steps  many steps in one launch, one workgroup per step: the table in LDS (n_classes <=
//                                 OEA_LOG_UNIFORM_STEPS_MAX_CLASSES), a status word per step instead of the host wait
// Both give the same values bit for bit.  Nothing here touches a gradient scratch: one object serves both builds of the library.
#include "row_ops.h"

namespace {

using oea::align256;

constexpr int kThreads = 1024;
constexpr int kPer = 4;        // tries per thread and chunk: one Philox call
constexpr int kChunk = kThreads * kPer;
constexpr int kLdsClasses = OEA_LOG_UNIFORM_STEPS_MAX_CLASSES;     // first[] in LDS: 32 KB

// The first-appearance table: first[c] holds ~t of the smallest try that drew c (0 = not drawn yet: an unsigned max).  What the two
// calls do differently with it is here; draw() is the rest.
struct GlobalTable {           // in the workspace, zero between calls: the drawn classes are listed in cls[] and cleared on the way out
    typedef int64_t idx_t;
    uint32_t *first;
    int32_t *cls;
    __device__ __forceinline__ void note(int64_t t, idx_t c) const {
        cls[t] = (int32_t)c;
        atomicMax(first + c, ~(uint32_t)t);
    }
    __device__ __forceinline__ void publish() const { __threadfence(); __syncthreads(); }
    __device__ __forceinline__ uint32_t read(int32_t c) const { return __hip_atomic_load(first + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ void clear(int64_t drawn) const {
        for (int64_t t = threadIdx.x; t < drawn; t += kThreads) first[cls[t]] = 0u;
    }
};
struct LdsTable {              // __shared__, zeroed by the kernel on entry: nothing to list, nothing to clear
    typedef int idx_t;
    uint32_t *first;
    __device__ __forceinline__ void note(int64_t t, idx_t c) const { atomicMax(first + c, ~(uint32_t)t); }
    __device__ __forceinline__ void publish() const { __syncthreads(); }
    __device__ __forceinline__ uint32_t read(int32_t c) const { return first[c]; }
    __device__ __forceinline__ void clear(int64_t) const {}
};

// One workgroup.  Try t of step s: word t & 3 of Philox(counter = (t >> 2, tag, step), key = seed), u = (w + 0.5) 2^-32, class =
// the first c with u < T[c].  A try is a first appearance when first[class] == ~t.  A block scan over the flags numbers the first
// appearances; the chunk in which their count reaches S ends the draw.  Returns the try that produced the S-th distinct class, -1
// when max_tries did not bring S of them.
template <class Table>
__device__ __forceinline__ int draw(const Table tab, typename Table::idx_t n_classes, int n_sampled, uint64_t seed, uint64_t step,
                                    const double *__restrict__ thr, int32_t *out_ids, int64_t max_tries) {
    __shared__ int wave_tot[kThreads / 64];
    __shared__ int s_found;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_found = -1;
    int have = 0;                    // distinct classes seen before this chunk (uniform)
    int64_t drawn = 0;
    __syncthreads();
    for (int64_t base = 0; base < max_tries; base += kChunk) {
        const int64_t t0 = base + (int64_t)tid * kPer;
        const uint4 w4 = oea::philox4x32_10((uint32_t)(t0 >> 2), 0x50726a45u, (uint32_t)step, (uint32_t)(step >> 32), (uint32_t)seed,
                                            (uint32_t)(seed >> 32));
        const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
        int32_t c[kPer];
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            const double u = ((double)w[i] + 0.5) * 2.3283064365386963e-10;
            typename Table::idx_t lo = 0, hi = n_classes - 1;          // first c with u < T[c]; T[E - 1] = 1 > u
            while (lo < hi) {
                const typename Table::idx_t mid = (lo + hi) >> 1;
                if (u < thr[mid]) hi = mid; else lo = mid + 1;
            }
            c[i] = (int32_t)lo;
            if (t0 + i < max_tries) tab.note(t0 + i, lo);
        }
        drawn = base + kChunk < max_tries ? base + kChunk : max_tries;
        tab.publish();
        int flag[kPer], mine = 0;
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            flag[i] = t0 + i < max_tries && tab.read(c[i]) == ~(uint32_t)(t0 + i);
            mine += flag[i];
        }
        int incl = mine;             // inclusive scan over the wave, then over the waves
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int v = __shfl_up(incl, off, 64);
            if (lane >= off) incl += v;
        }
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        int before = have, total = have;
        for (int wv = 0; wv < kThreads / 64; ++wv) {
            if (wv < wave) before += wave_tot[wv];
            total += wave_tot[wv];
        }
        int rank = before + incl - mine;           // first appearances in front of this thread's tries
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            if (flag[i]) {
                if (rank < n_sampled) out_ids[rank] = c[i];
                if (rank == n_sampled - 1) s_found = (int)(t0 + i);
                ++rank;
            }
        }
        have = total;
        __syncthreads();
        if (have >= n_sampled) break;
    }
    tab.clear(drawn);
    return s_found;
}

// the successful end of a draw: the status word, num_tries, log Q of every id
__device__ __forceinline__ void finish(int found, double n_classes, int n_sampled, const int32_t *out_ids, float *out_logq,
                                       int64_t *out_tries, int32_t *status) {
    const int tid = threadIdx.x;
    const double n_tries = (double)(found + 1), inv = 1.0 / log(n_classes + 1.0);
    if (tid == 0) { *status = 0; *out_tries = found + 1; }
    __threadfence();
    __syncthreads();
    for (int j = tid; j < n_sampled; j += kThreads)
        out_logq[j] = (float)oea::row::log_q(__hip_atomic_load(out_ids + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), n_tries, inv);
}

__global__ __launch_bounds__(kThreads) void sample_kernel(int64_t n_classes, int n_sampled, uint64_t seed, uint64_t step,
                                                          const double *__restrict__ thr, int32_t *out_ids, int64_t *out_tries,
                                                          float *out_logq, uint32_t *first, int32_t *cls, int32_t *status,
                                                          int64_t max_tries) {
    const int found = draw(GlobalTable{first, cls}, n_classes, n_sampled, seed, step, thr, out_ids, max_tries);
    if (found < 0) {
        if (threadIdx.x == 0) *status = 1;
        return;
    }
    finish(found, (double)n_classes, n_sampled, out_ids, out_logq, out_tries, status);
}

__global__ __launch_bounds__(kThreads) void sample_steps_kernel(int n_classes, int n_sampled, uint64_t seed, uint64_t step0,
                                                                const double *__restrict__ thr, int32_t *out_ids_all,
                                                                int64_t *out_tries_all, float *out_logq_all, int32_t *status_all,
                                                                int64_t max_tries) {
    __shared__ uint32_t first[kLdsClasses];
    const int tid = threadIdx.x;
    int32_t *out_ids = out_ids_all + (int64_t)blockIdx.x * n_sampled;
    float *out_logq = out_logq_all + (int64_t)blockIdx.x * n_sampled;
    for (int c = tid; c < n_classes; c += kThreads) first[c] = 0u;
    const int found = draw(LdsTable{first}, n_classes, n_sampled, seed, step0 + blockIdx.x, thr, out_ids, max_tries);
    if (found < 0) {        // not reached in 64 S tries: valid ids all the same (a caller that ignores the status stays in bounds)
        for (int j = tid; j < n_sampled; j += kThreads) { out_ids[j] = j; out_logq[j] = 0.f; }
        if (tid == 0) { status_all[blockIdx.x] = 1; out_tries_all[blockIdx.x] = 1; }
        return;
    }
    finish(found, (double)n_classes, n_sampled, out_ids, out_logq, out_tries_all + blockIdx.x, status_all + blockIdx.x);
}

}  // namespace

extern "C" {

size_t oea_log_uniform_workspace_bytes(int64_t n_classes, int64_t n_sampled) {
    if (n_classes < 1 || n_sampled < 1) return 0;
    return align256(4 * (size_t)n_classes) + align256(4 * ((size_t)64 * n_sampled + kChunk)) + 256;
}

int oea_log_uniform_sample(int64_t n_classes, int64_t n_sampled, uint64_t seed, uint64_t step, const double *thresholds,
                           int32_t *out_ids, int64_t *out_num_tries, float *out_log_q_sampled, void *workspace, void *stream) {
    OEA_REQUIRE(thresholds && out_ids && out_num_tries && out_log_q_sampled && workspace, "null pointer");
    OEA_REQUIRE(n_sampled >= 1 && n_sampled <= n_classes, "1 <= n_sampled <= n_classes");
    OEA_REQUIRE(n_classes < (1LL << 31) && n_sampled < (1LL << 24), "n_classes < 2^31, n_sampled < 2^24");
    hipStream_t st = oea::as_stream(stream);
    char *b = static_cast<char *>(workspace);
    uint32_t *first = reinterpret_cast<uint32_t *>(b);
    int32_t *cls = reinterpret_cast<int32_t *>(b + align256(4 * (size_t)n_classes));
    int32_t *status = reinterpret_cast<int32_t *>(b + oea_log_uniform_workspace_bytes(n_classes, n_sampled) - 256);
    sample_kernel<<<1, kThreads, 0, st>>>(n_classes, (int)n_sampled, seed, step, thresholds, out_ids, out_num_tries, out_log_q_sampled,
                                          first, cls, status, 64 * n_sampled);
    OEA_CHECK_HIP(hipGetLastError());
    int32_t host_status = 0;
    OEA_CHECK_HIP(hipMemcpyAsync(&host_status, status, sizeof(host_status), hipMemcpyDeviceToHost, st));
    OEA_CHECK_HIP(hipStreamSynchronize(st));
    if (host_status != 0) {
        oea::set_error("oea_log_uniform_sample: %lld distinct classes of %lld not reached in %lld tries", (long long)n_sampled,
                       (long long)n_classes, (long long)(64 * n_sampled));
        return OEA_EUNSUPPORTED;
    }
    return OEA_OK;
}

int oea_log_uniform_sample_steps(int64_t n_classes, int64_t n_sampled, uint64_t seed, uint64_t step0, int64_t n_steps,
                                 const double *thresholds, int32_t *out_ids, int64_t *out_num_tries, float *out_log_q_sampled,
                                 int32_t *status, void *stream) {
    OEA_REQUIRE(thresholds && out_ids && out_num_tries && out_log_q_sampled && status, "null pointer");
    OEA_REQUIRE(n_sampled >= 1 && n_sampled <= n_classes && n_steps >= 0 && n_steps < ((int64_t)1 << 31), "1 <= n_sampled <= n_classes, n_steps");
    if (n_classes > kLdsClasses) {
        oea::set_error("oea_log_uniform_sample_steps: n_classes %lld > %d (the first-appearance table lives in LDS; "
                       "oea_log_uniform_sample has no limit)", (long long)n_classes, kLdsClasses);
        return OEA_EUNSUPPORTED;
    }
    if (n_steps == 0) return OEA_OK;
    sample_steps_kernel<<<(unsigned)n_steps, kThreads, 0, oea::as_stream(stream)>>>(
        (int)n_classes, (int)n_sampled, seed, step0, thresholds, out_ids, out_num_tries, out_log_q_sampled, status, 64 * n_sampled);
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

}  // extern "C"
