// sim_csr.hip -- JAPE's attribute similarity as a CSR, and the similarity loss over it (approaches/jape.py:86-98, 127-149).
//
// The reference keeps sim_mat = ref1_attr . ref2_attr^T dense ([n_ref, n_ref] fp32, 25.6 GB at the 100K split) and zeroes what
// lies below attr_sim_mat_threshold (jape.py:148).  Here the matrix exists one block of rows at a time: oea_sim_matrix(inner)
// into the caller's block buffer, then one wave per row keeps the entries >= threshold.  Two passes, once per run:
//   oea_sim_csr_count   the kept entries of every row, then indptr = their exclusive scan (indptr[n1] = nnz; the caller reads
//                       that one word back to size col / val)
//   oea_sim_csr_fill    the same blocks again; a wave walks its row 64 columns at a time and places the kept ones with a ballot
//                       prefix, so the columns of a row ascend.  A write is bounded by the row's own indptr range.
// The two passes ASSUME that oea_sim_matrix gives the same bits when it is called twice on the same operands.  Were that ever
// lost, a row could keep another number of entries in the second pass than in the first; the bound
// above keeps that from writing outside the row, and fill_rows_kernel counts such rows in *mismatch so that the caller sees it.
// oea_jape_sim_loss: one wave per sampled row, everything in fp64 (a row of the matrix may hold hundreds of entries):
//   t = sum_j val_ij l2n(ent)[ref2_ids[col_ij]],  loss += beta | l2n(ent)[ref1_ids[rows[i]]] - l2n(t) |^2,  l2n(0) = 0.
// Nothing is written but loss_accum: the reference builds sim_optimizer and never runs it (jape.py:136 fetches sim_loss alone).
#include "common.h"

#include <algorithm>

namespace {

constexpr int kWaves = 4;
constexpr int kMaxDim = 128;

__global__ __launch_bounds__(64 * kWaves) void count_rows_kernel(const float *__restrict__ block, int64_t rows, int64_t n2, float thr,
                                                                 int64_t *__restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float *s = block + r * n2;
    int c = 0;
    for (int64_t j = lane; j < n2; j += 64) c += s[j] >= thr ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    if (lane == 0) counts[r] = c;
}

// exclusive scan of counts[0 .. n] in place by one workgroup (counts[n] is overwritten with the total); n is a few 10^4
__global__ __launch_bounds__(1024) void scan_kernel(int64_t *__restrict__ v, int64_t n) {
    __shared__ int64_t part[1024];
    const int t = threadIdx.x;
    const int64_t per = (n + 1023) / 1024, lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    int64_t s = 0;
    for (int64_t i = lo; i < hi; ++i) s += v[i];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        int64_t run = 0;
        for (int i = 0; i < 1024; ++i) { const int64_t x = part[i]; part[i] = run; run += x; }
        v[n] = run;
    }
    __syncthreads();
    int64_t run = part[t];
    for (int64_t i = lo; i < hi; ++i) { const int64_t x = v[i]; v[i] = run; run += x; }
}

__global__ __launch_bounds__(64 * kWaves) void fill_rows_kernel(const float *__restrict__ block, int64_t rows, int64_t n2, float thr,
                                                                const int64_t *__restrict__ indptr, int32_t *__restrict__ col,
                                                                float *__restrict__ val, int32_t *__restrict__ mismatch) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float *s = block + r * n2;
    int64_t at = indptr[r];
    const int64_t end = indptr[r + 1];
    for (int64_t j0 = 0; j0 < n2; j0 += 64) {
        const int64_t j = j0 + lane;
        const float x = j < n2 ? s[j] : 0.f;
        const bool keep = j < n2 && x >= thr;
        const unsigned long long mask = __ballot(keep);
        const int64_t p = at + __popcll(mask & ((1ull << lane) - 1ull));
        if (keep && p < end) { col[p] = (int32_t)j; val[p] = x; }
        at += __popcll(mask);
    }
    if (lane == 0 && at != end) atomicAdd(mismatch, 1);
}

struct SimLossArgs {
    const float *ent;
    int ld, dim;
    const int32_t *ref1_ids, *ref2_ids, *rows, *col;
    const int64_t *indptr;
    const float *val;
    int64_t m;
    double beta;
    double *loss_accum;
};

// columns 2 lane, 2 lane + 1 of l2n(row) in fp64 (zero from dim on)
__device__ __forceinline__ void load_l2n(const float *row, int dim, int lane, double &x, double &y) {
    const int c = 2 * lane;
    x = 0.0; y = 0.0;
    if (c < dim) {
        const float2 v = *reinterpret_cast<const float2 *>(row + c);
        x = v.x;
        if (c + 1 < dim) y = v.y;
    }
    const double inv = 1.0 / sqrt(fmax(oea::wave_sum_d(x * x + y * y), 1e-12));
    x *= inv; y *= inv;
}

__global__ __launch_bounds__(64 * kWaves) void sim_loss_kernel(SimLossArgs A) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double loss_local = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kWaves + wave; i < A.m; i += (int64_t)gridDim.x * kWaves) {
        const int64_t r = A.rows[i];
        double tx = 0.0, ty = 0.0;
        for (int64_t e = A.indptr[r]; e < A.indptr[r + 1]; ++e) {
            double x, y;
            load_l2n(A.ent + (int64_t)A.ref2_ids[A.col[e]] * A.ld, A.dim, lane, x, y);
            const double v = A.val[e];
            tx += v * x; ty += v * y;
        }
        const double inv = 1.0 / sqrt(fmax(oea::wave_sum_d(tx * tx + ty * ty), 1e-12));
        double ax, ay;
        load_l2n(A.ent + (int64_t)A.ref1_ids[r] * A.ld, A.dim, lane, ax, ay);
        const double dx = ax - tx * inv, dy = ay - ty * inv;
        loss_local += oea::wave_sum_d(dx * dx + dy * dy);
    }
    oea::block_loss_add<kWaves>(loss_local, lane, wave, A.loss_accum, A.beta);
}

// one pass over the row blocks of e1: similarity into block_buf, then the counting or the filling kernel
int sweep(const float *e1, int64_t n1, int32_t ld1, const float *e2, int64_t n2, int32_t ld2, int32_t dim, float threshold,
          int64_t block_rows, float *block_buf, int64_t *indptr, int32_t *col, float *val, int32_t *mismatch, hipStream_t st) {
    for (int64_t r0 = 0; r0 < n1; r0 += block_rows) {
        const int64_t rows = std::min(block_rows, n1 - r0);
        const int rc = oea_sim_matrix(e1 + r0 * ld1, rows, ld1, e2, n2, ld2, dim, OEA_METRIC_INNER, block_buf, n2, st);
        if (rc != OEA_OK) return rc;
        const unsigned grid = (unsigned)oea::ceil_div(rows, kWaves);
        if (col) fill_rows_kernel<<<grid, 64 * kWaves, 0, st>>>(block_buf, rows, n2, threshold, indptr + r0, col, val, mismatch);
        else count_rows_kernel<<<grid, 64 * kWaves, 0, st>>>(block_buf, rows, n2, threshold, indptr + r0);
        OEA_CHECK_HIP(hipGetLastError());
    }
    return OEA_OK;
}

int check_csr_args(const float *e1, int64_t n1, int32_t ld1, const float *e2, int64_t n2, int32_t ld2, int32_t dim, float threshold,
                   int64_t block_rows, const float *block_buf, const int64_t *indptr) {
    OEA_REQUIRE(e1 && e2 && block_buf && indptr, "null pointer");
    OEA_REQUIRE(n1 >= 1 && n2 >= 1 && n2 < ((int64_t)1 << 31) && block_rows >= 1, "n1, n2, block_rows >= 1 and n2 < 2^31");
    OEA_REQUIRE(dim > 0 && dim <= ld1 && dim <= ld2 && ld1 % 4 == 0 && ld2 % 4 == 0, "0 < dim <= ld, ld % 4 == 0");
    OEA_REQUIRE(threshold == threshold, "threshold is NaN");
    return OEA_OK;
}

}  // namespace

extern "C" {

int oea_sim_csr_count(const float *e1, int64_t n1, int32_t ld1, const float *e2, int64_t n2, int32_t ld2, int32_t dim, float threshold,
                      int64_t block_rows, float *block_buf, int64_t *indptr, void *stream) {
    const int rc = check_csr_args(e1, n1, ld1, e2, n2, ld2, dim, threshold, block_rows, block_buf, indptr);
    if (rc != OEA_OK) return rc;
    hipStream_t st = oea::as_stream(stream);
    const int rs = sweep(e1, n1, ld1, e2, n2, ld2, dim, threshold, block_rows, block_buf, indptr, nullptr, nullptr, nullptr, st);
    if (rs != OEA_OK) return rs;
    scan_kernel<<<1, 1024, 0, st>>>(indptr, n1);
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

int oea_sim_csr_fill(const float *e1, int64_t n1, int32_t ld1, const float *e2, int64_t n2, int32_t ld2, int32_t dim, float threshold,
                     int64_t block_rows, float *block_buf, const int64_t *indptr, int32_t *col, float *val, int32_t *mismatch,
                     void *stream) {
    const int rc = check_csr_args(e1, n1, ld1, e2, n2, ld2, dim, threshold, block_rows, block_buf, indptr);
    if (rc != OEA_OK) return rc;
    OEA_REQUIRE(col && val && mismatch, "null pointer");
    return sweep(e1, n1, ld1, e2, n2, ld2, dim, threshold, block_rows, block_buf, const_cast<int64_t *>(indptr), col, val, mismatch,
                 oea::as_stream(stream));
}

int oea_jape_sim_loss(const float *ent, int64_t n_ent, int32_t dim, int32_t ld, const int32_t *ref1_ids, int64_t n_ref1,
                      const int32_t *ref2_ids, int64_t n_ref2, const int64_t *indptr, const int32_t *col, const float *val,
                      const int32_t *rows, int64_t m, float beta, double *loss_accum, void *stream) {
    OEA_REQUIRE(ent && ref1_ids && ref2_ids && indptr && col && val && loss_accum && (rows || m == 0), "null pointer");
    OEA_REQUIRE(n_ent >= 1 && n_ref1 >= 1 && n_ref2 >= 1 && m >= 0, "sizes");
    OEA_REQUIRE(ld % 4 == 0, "ld % 4 == 0");
    OEA_REQUIRE(dim > 0 && dim <= ld, "0 < dim <= ld");
    if (dim > kMaxDim) {
        oea::set_error("oea_jape_sim_loss: dim %d > %d", dim, kMaxDim);
        return OEA_EUNSUPPORTED;
    }
    if (m == 0) return OEA_OK;
    SimLossArgs A;
    A.ent = ent; A.ld = ld; A.dim = dim;
    A.ref1_ids = ref1_ids; A.ref2_ids = ref2_ids; A.rows = rows; A.col = col;
    A.indptr = indptr; A.val = val; A.m = m; A.beta = (double)beta; A.loss_accum = loss_accum;
    const unsigned grid = (unsigned)std::min<int64_t>(oea::ceil_div(m, kWaves), 2048);
    sim_loss_kernel<<<grid, 64 * kWaves, 0, oea::as_stream(stream)>>>(A);
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

}  // extern "C"
