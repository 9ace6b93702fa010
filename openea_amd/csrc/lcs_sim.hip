// lcs_sim.hip -- IMUSE's attribute-value string similarity (approaches/imuse.py:42-66, 195-249).
//
// Levenshtein.ratio(a, b) = (|a| + |b| - d) / (|a| + |b|) with d the edit distance at substitution cost 2, which is
//     ratio(a, b) = 2 LCS(a, b) / (|a| + |b|)      over code points, 1.0 when both strings are empty.
// LCS by the bit-vector recurrence: the pattern's positions are the bits of V (W 64-bit words, W = 1, 2 or 4), PM[c] the mask of the
// pattern positions that hold c, and per text character
//     u = V & PM[c];   V = (V + u) | (V - u);          LCS = popcount(~V)
// The add carries from word to word.  The subtract never borrows, because u is a subset of V's bits: V - u = V & ~PM[c] word by word.
//
// A STRING POOL is the distinct strings of one KG side as int32 code points back to back (UTF-32, never UTF-8: the reference
// compares the elements of a Python str) with int64 offsets [n_str + 1].
//
// PM lives in LDS as an open-addressed table keyed by code point: a slot is W + 1 64-bit words, the key and then its masks.
// max(16, the power of two >= 2 m) slots for a pattern of m code points: the table is at most half full and a probe ends at the
// key or at an empty slot, whose masks are zero.
//   lcs_pairs_kernel          one wave per pair, the shorter string as the pattern; every lane walks the same text.
//   attr_sim_records_kernel   one workgroup (4 waves) per row i of KG1.  The tables of the row's K values are built once into a 20 KB
//                             arena and stay there for the whole walk over the columns; a lane owns a column j and runs its K texts
//                             against them, s = (sum of the ratios in the order of k) / count in fp64 as imuse.py:52-59 does.  Then a
//                             prefix maximum over the 256 columns of the block, carried from block to block, leaves the RECORDS:
//                             the (j, s) with s > threshold and s > every earlier s of the row -- all run_one_ea reads of the row.
// What does not take the table -- a pattern above 256 code points, or a row whose tables do not fit the arena -- goes to
// wave_lcs: the row-wise DP  cur[j] = prefixmax_j max(prev[j], prev[j - 1] + [a_i == b_j])  by the whole wave, 64 columns a step, the
// longer string along the row: in registers up to 512 columns, in the caller's workspace beyond.  Slower, and exact.
//
// What lives in device memory cannot be refused by the return status without a host synchronisation.  So every call first runs
// check kernels over the offsets and the indices it was given; they set bits in *err_flag (the caller zeroes it), and the kernels
// that follow on the stream write nothing once it is non-zero.
#include "common.h"

#include <algorithm>

namespace {

constexpr int kArenaWords = 2560;                    // 20 KB of 64-bit words: ten tables of patterns <= 64 (128 slots x 16 B)
constexpr int kMaxK = 32;
constexpr int kRecWaves = 4;
constexpr int kLcsGrid = 2048;                       // workgroups of either kernel, and so workspace rows (x kRecWaves)
constexpr uint32_t kEmpty = 0xFFFFFFFFu;             // no code point: they end at 0x10FFFF

enum { ERR_POOL = 1, ERR_INDEX = 2 };

struct Pool {
    const int32_t *cp;
    const int64_t *off;
    int64_t n_str, n_cp;
};

__device__ __forceinline__ int words_of(int m) { return m <= 64 ? 1 : m <= 128 ? 2 : m <= 256 ? 4 : 0; }
__device__ __forceinline__ int slots_log2_of(int m) {
    int lg = 4;
    while ((1 << lg) < 2 * m) ++lg;
    return lg;
}
__device__ __forceinline__ uint32_t slot_of(uint32_t c, int lg) { return (c * 0x9E3779B1u) >> (32 - lg); }

// the table of pat[0 .. m) into tab, by every thread of the workgroup (the caller puts a barrier before the first probe)
template <int W>
__device__ void build_table(unsigned long long *tab, int lg, const int32_t *pat, int m) {
    const int slots = 1 << lg;
    for (int i = threadIdx.x; i < slots * (W + 1); i += blockDim.x) tab[i] = i % (W + 1) == 0 ? (unsigned long long)kEmpty : 0ull;
    __syncthreads();
    for (int p = threadIdx.x; p < m; p += blockDim.x) {
        const uint32_t c = (uint32_t)pat[p];
        uint32_t s = slot_of(c, lg);
        for (;;) {
            const uint32_t was = atomicCAS(reinterpret_cast<uint32_t *>(tab + (size_t)s * (W + 1)), kEmpty, c);
            if (was == kEmpty || was == c) break;
            s = (s + 1) & (slots - 1);
        }
        atomicOr(tab + (size_t)s * (W + 1) + 1 + (p >> 6), 1ull << (p & 63));
    }
}

// LCS(pattern of the table, text[0 .. n)) by one lane
template <int W>
__device__ __forceinline__ int lcs_bits(const unsigned long long *tab, int lg, const int32_t *text, int n) {
    unsigned long long V[W];
#pragma unroll
    for (int w = 0; w < W; ++w) V[w] = ~0ull;
    const uint32_t mask = (1u << lg) - 1u;
    uint32_t c = n > 0 ? (uint32_t)text[0] : 0u;
    for (int t = 0; t < n; ++t) {
        const uint32_t next = (uint32_t)text[t + 1 < n ? t + 1 : t];         // no branch: this load is under way while c is used
        uint32_t s = slot_of(c, lg);
        unsigned long long pm[W];
        for (;;) {
            const unsigned long long *slot = tab + (size_t)s * (W + 1);
            const uint32_t key = (uint32_t)slot[0];
#pragma unroll
            for (int w = 0; w < W; ++w) pm[w] = slot[1 + w];
            if (key == c || key == kEmpty) break;
            s = (s + 1) & mask;
        }
        unsigned long long carry = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const unsigned long long u = V[w] & pm[w];
            const unsigned long long a = V[w] + u, b = a + carry;
            carry = (unsigned long long)(a < u) | (unsigned long long)(b < a);
            V[w] = b | (V[w] & ~pm[w]);
        }
        c = next;
    }
    int lcs = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) lcs += __popcll(~V[w]);
    return lcs;
}

__device__ __forceinline__ int lcs_bits_any(int W, const unsigned long long *tab, int lg, const int32_t *text, int n) {
    return W == 1 ? lcs_bits<1>(tab, lg, text, n) : W == 2 ? lcs_bits<2>(tab, lg, text, n) : lcs_bits<4>(tab, lg, text, n);
}

__device__ void build_table_any(int W, unsigned long long *tab, int lg, const int32_t *pat, int m) {
    if (W == 1) build_table<1>(tab, lg, pat, m);
    else if (W == 2) build_table<2>(tab, lg, pat, m);
    else build_table<4>(tab, lg, pat, m);
}

// LCS(a[0 .. la), b[0 .. lb)) by the whole wave, any lengths; row: lb + 1 ints of this wave's own.  A row element is read and
// written by one lane only (column j by lane (j - 1) % 64); its left neighbour comes through the lanes, not through memory.
__device__ int wave_lcs_dp(const int32_t *a, int la, const int32_t *b, int lb, int32_t *row, int lane) {
    if (la == 0 || lb == 0) return 0;
    for (int j = 1 + lane; j <= lb; j += 64) row[j] = 0;
    int run = 0;
    for (int i = 0; i < la; ++i) {
        const int32_t ca = a[i];
        int left = 0;                    // prev[j0 - 1]
        run = 0;                         // cur[j0 - 1]
        for (int j0 = 1; j0 <= lb; j0 += 64) {
            const int j = j0 + lane;
            const bool valid = j <= lb;
            const int pj = valid ? row[j] : 0;
            int pl = __shfl_up(pj, 1, 64);
            if (lane == 0) pl = left;
            int t = valid ? max(pj, pl + (b[j - 1] == ca ? 1 : 0)) : 0;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int x = __shfl_up(t, off, 64);
                if (lane >= off) t = max(t, x);
            }
            t = max(t, run);
            if (valid) row[j] = t;
            left = __shfl(pj, 63, 64);
            run = __shfl(t, 63, 64);
        }
    }
    return run;
}

// The same DP with the row in registers: lane l keeps columns l, l + 64, ... of the longer string b (lb <= 64 R) and b's code points
// at those columns, so a step over 64 columns is shuffles and compares with no memory in it.
template <int R>
__device__ int wave_lcs_dp_reg(const int32_t *a, int la, const int32_t *b, int lb, int lane) {
    if (la == 0 || lb == 0) return 0;
    int row[R], bc[R];
#pragma unroll
    for (int c = 0; c < R; ++c) {
        row[c] = 0;
        bc[c] = c * 64 + lane < lb ? b[c * 64 + lane] : 0;
    }
    int run = 0;
    int32_t ca = a[0];
    for (int i = 0; i < la; ++i) {
        const int32_t next = a[i + 1 < la ? i + 1 : i];
        int left = 0;
        run = 0;
#pragma unroll
        for (int c = 0; c < R; ++c) {
            if (c * 64 < lb) {                                   // the same in every lane
                const bool valid = c * 64 + lane < lb;
                const int pj = row[c];
                int pl = __shfl_up(pj, 1, 64);
                if (lane == 0) pl = left;
                int t = valid ? max(pj, pl + (bc[c] == ca ? 1 : 0)) : 0;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const int x = __shfl_up(t, off, 64);
                    if (lane >= off) t = max(t, x);
                }
                t = max(t, run);
                row[c] = valid ? t : 0;
                left = __shfl(pj, 63, 64);
                run = __shfl(t, 63, 64);
            }
        }
        ca = next;
    }
    return run;
}

constexpr int kDpRegs = 8;                           // the DP row lives in registers up to 512 columns

// LCS of two strings of any lengths by the whole wave: the longer one along the DP row
__device__ __forceinline__ int wave_lcs(const int32_t *a, int la, const int32_t *b, int lb, int32_t *row, int lane) {
    if (la > lb) {
        const int32_t *p = a; a = b; b = p;
        const int n = la; la = lb; lb = n;
    }
    return lb <= 64 * kDpRegs ? wave_lcs_dp_reg<kDpRegs>(a, la, b, lb, lane) : wave_lcs_dp(a, la, b, lb, row, lane);
}

__device__ __forceinline__ double ratio_of(int lcs, int l1, int l2) {
    const int tot = l1 + l2;
    return tot > 0 ? (double)(2 * lcs) / (double)tot : 1.0;
}

// ---- checks of what lies in device memory ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void check_pool_kernel(Pool p, int64_t max_len, int32_t *err) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (i == 0) bad = p.off[0] != 0 || p.off[p.n_str] != p.n_cp;
    if (i < p.n_str) {
        const int64_t d = p.off[i + 1] - p.off[i];
        bad = bad || d < 0 || d > max_len;
    }
    if (bad) atomicOr(err, ERR_POOL);
}

// v[0 .. n) in [lo, hi); stride 2 with two bounds walks the two columns of a pair list
__global__ __launch_bounds__(256) void check_index_kernel(const int32_t *v, int64_t n, int64_t lo, int64_t hi, int32_t *err) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && (v[i] < lo || v[i] >= hi)) atomicOr(err, ERR_INDEX);
}
__global__ __launch_bounds__(256) void check_pairs_kernel(const int32_t *pairs, int64_t n, int64_t hi1, int64_t hi2, int32_t *err) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && (pairs[2 * i] < 0 || pairs[2 * i] >= hi1 || pairs[2 * i + 1] < 0 || pairs[2 * i + 1] >= hi2)) atomicOr(err, ERR_INDEX);
}

// ---- pairs -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void lcs_pairs_kernel(Pool p1, Pool p2, const int32_t *__restrict__ pairs, int64_t n,
                                                       int32_t *__restrict__ lcs_out, double *__restrict__ ratio_out,
                                                       int32_t *__restrict__ ws, int64_t ws_stride, const int32_t *err) {
    __shared__ unsigned long long arena[kArenaWords];
    if (*err != 0) return;
    const int lane = threadIdx.x;
    int32_t *row = ws + (int64_t)blockIdx.x * ws_stride;
    for (int64_t q = blockIdx.x; q < n; q += gridDim.x) {
        const int64_t s1 = p1.off[pairs[2 * q]], s2 = p2.off[pairs[2 * q + 1]];
        const int l1 = (int)(p1.off[pairs[2 * q] + 1] - s1), l2 = (int)(p2.off[pairs[2 * q + 1] + 1] - s2);
        const bool first_short = l1 <= l2;
        const int32_t *pat = first_short ? p1.cp + s1 : p2.cp + s2, *text = first_short ? p2.cp + s2 : p1.cp + s1;
        const int m = first_short ? l1 : l2, nt = first_short ? l2 : l1;
        const int W = words_of(m);
        int lcs;
        if (W) {
            const int lg = slots_log2_of(m);
            __syncthreads();                                     // the previous pair's probes are over
            build_table_any(W, arena, lg, pat, m);
            __syncthreads();
            lcs = lcs_bits_any(W, arena, lg, text, nt);
        } else {
            lcs = wave_lcs(pat, m, text, nt, row, lane);
        }
        if (lane == 0) {
            lcs_out[q] = lcs;
            ratio_out[q] = ratio_of(lcs, l1, l2);
        }
    }
}

// ---- records ---------------------------------------------------------------------------------------------------------------------------
struct RecArgs {
    Pool p1, p2;
    int32_t K, cap;
    const int32_t *idx1, *idx2, *rows;
    int64_t n1, n2, n_rows;
    double threshold;
    int32_t *rec_col, *rec_cnt, *overflow, *ws;
    double *rec_val;
    int64_t ws_stride;
    const int32_t *err;
};

__global__ __launch_bounds__(64 * kRecWaves) void attr_sim_records_kernel(RecArgs A) {
    __shared__ unsigned long long arena[kArenaWords];
    __shared__ int64_t s_start[kMaxK];
    __shared__ int s_len[kMaxK], s_words[kMaxK], s_lg[kMaxK], s_at[kMaxK];      // s_words: 0 absent, -1 generic, else W
    __shared__ double s_wave_max[kRecWaves];
    __shared__ int s_wave_cnt[kRecWaves];
    if (*A.err != 0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int32_t *dp_row = A.ws + ((int64_t)blockIdx.x * kRecWaves + wave) * A.ws_stride;
    for (int64_t r = blockIdx.x; r < A.n_rows; r += gridDim.x) {
        const int64_t i = A.rows ? A.rows[r] : r;
        __syncthreads();                                         // the previous row's probes are over
        if (threadIdx.x == 0) {
            int used = 0;
            for (int k = 0; k < A.K; ++k) {
                const int32_t v = A.idx1[(int64_t)k * A.n1 + i];
                s_words[k] = 0;
                if (v < 0) continue;
                s_start[k] = A.p1.off[v];
                const int m = (int)(A.p1.off[v + 1] - s_start[k]);
                s_len[k] = m;
                const int W = words_of(m), lg = slots_log2_of(W ? m : 0), need = (W + 1) << lg;
                if (W && used + need <= kArenaWords) {
                    s_words[k] = W; s_lg[k] = lg; s_at[k] = used;
                    used += need;
                } else {
                    s_words[k] = -1;
                }
            }
        }
        __syncthreads();
        for (int k = 0; k < A.K; ++k)
            if (s_words[k] > 0) build_table_any(s_words[k], arena + s_at[k], s_lg[k], A.p1.cp + s_start[k], s_len[k]);
        __syncthreads();

        double run = A.threshold;                               // the row's sim_max (imuse.py:50)
        int cnt = 0;
        for (int64_t j0 = 0; j0 < A.n2; j0 += 64 * kRecWaves) {
            const int64_t j = j0 + threadIdx.x;
            const bool valid = j < A.n2;
            double s = 0.0;
            int c = 0;
            for (int k = 0; k < A.K; ++k) {
                const int W = s_words[k];
                if (W == 0) continue;
                const int32_t v2 = valid ? A.idx2[(int64_t)k * A.n2 + j] : -1;
                const bool has = v2 >= 0;
                int64_t t0 = 0;
                int nt = 0, lcs = 0;
                if (has) {
                    t0 = A.p2.off[v2];
                    nt = (int)(A.p2.off[v2 + 1] - t0);
                }
                if (W > 0) {
                    if (has) lcs = lcs_bits_any(W, arena + s_at[k], s_lg[k], A.p2.cp + t0, nt);
                } else {                                         // the wave takes its lanes' pairs one after the other
                    unsigned long long todo = __ballot(has);
                    while (todo) {
                        const int l = __ffsll((long long)todo) - 1;
                        todo &= todo - 1;
                        const int64_t bt = __shfl(t0, l, 64);
                        const int bn = __shfl(nt, l, 64);
                        const int x = wave_lcs(A.p1.cp + s_start[k], s_len[k], A.p2.cp + bt, bn, dp_row, lane);
                        if (lane == l) lcs = x;
                    }
                }
                if (has) {
                    s += ratio_of(lcs, s_len[k], nt);
                    ++c;
                }
            }
            if (c > 0) s /= (double)c;

            // records of these 256 columns: s above the running maximum and above everything to its left
            const double x = valid ? s : -HUGE_VAL;
            double incl = x;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const double y = __shfl_up(incl, off, 64);
                if (lane >= off) incl = fmax(incl, y);
            }
            double before = __shfl_up(incl, 1, 64);
            if (lane == 0) before = -HUGE_VAL;
            if (lane == 63) s_wave_max[wave] = incl;
            __syncthreads();
            before = fmax(before, run);
            for (int w = 0; w < wave; ++w) before = fmax(before, s_wave_max[w]);
            const bool is_rec = valid && x > before;
            const unsigned long long m = __ballot(is_rec);
            if (lane == 0) s_wave_cnt[wave] = __popcll(m);
            __syncthreads();
            int pos = cnt + __popcll(m & ((1ull << lane) - 1ull));
            for (int w = 0; w < wave; ++w) pos += s_wave_cnt[w];
            if (is_rec && pos < A.cap) {
                A.rec_col[r * A.cap + pos] = (int32_t)j;
                A.rec_val[r * A.cap + pos] = x;
            }
            for (int w = 0; w < kRecWaves; ++w) {
                cnt += s_wave_cnt[w];
                run = fmax(run, s_wave_max[w]);
            }
            __syncthreads();                                     // s_wave_* are free for the next block of columns
        }
        if (threadIdx.x == 0) {
            A.rec_cnt[r] = min(cnt, A.cap);
            A.overflow[r] = cnt > A.cap ? 1 : 0;
        }
    }
}

int check_pools(const Pool &p1, const Pool &p2, int64_t max_len) {
    OEA_REQUIRE(p1.off && p2.off, "null pointer");
    OEA_REQUIRE(p1.n_str >= 1 && p2.n_str >= 1 && p1.n_cp >= 0 && p2.n_cp >= 0, "a pool holds n_str >= 1 strings of n_cp >= 0 code points");
    OEA_REQUIRE((p1.cp || p1.n_cp == 0) && (p2.cp || p2.n_cp == 0), "null pointer");
    OEA_REQUIRE(p1.n_str < ((int64_t)1 << 31) && p2.n_str < ((int64_t)1 << 31), "n_str < 2^31");
    OEA_REQUIRE(max_len >= 0 && max_len < ((int64_t)1 << 30), "0 <= max_len < 2^30");
    return OEA_OK;
}

int launch_pool_checks(const Pool &p1, const Pool &p2, int64_t max_len, int32_t *err, hipStream_t st) {
    check_pool_kernel<<<(unsigned)oea::ceil_div(p1.n_str, 256), 256, 0, st>>>(p1, max_len, err);
    OEA_CHECK_HIP(hipGetLastError());
    check_pool_kernel<<<(unsigned)oea::ceil_div(p2.n_str, 256), 256, 0, st>>>(p2, max_len, err);
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

}  // namespace

extern "C" {

size_t oea_lcs_workspace_ints(int64_t max_len) {
    return max_len < 0 ? 0 : (size_t)kLcsGrid * kRecWaves * (size_t)(max_len + 1);
}

int oea_lcs_ratio_pairs(const int32_t *cp1, const int64_t *off1, int64_t n_str1, int64_t n_cp1, const int32_t *cp2, const int64_t *off2,
                        int64_t n_str2, int64_t n_cp2, int64_t max_len, const int32_t *pairs, int64_t n, int32_t *lcs, double *ratio,
                        int32_t *workspace, int32_t *err_flag, void *stream) {
    const Pool p1{cp1, off1, n_str1, n_cp1}, p2{cp2, off2, n_str2, n_cp2};
    const int rc = check_pools(p1, p2, max_len);
    if (rc != OEA_OK) return rc;
    OEA_REQUIRE(n >= 0, "n >= 0");
    OEA_REQUIRE(workspace && err_flag && ((pairs && lcs && ratio) || n == 0), "null pointer");
    if (n == 0) return OEA_OK;
    hipStream_t st = oea::as_stream(stream);
    const int rp = launch_pool_checks(p1, p2, max_len, err_flag, st);
    if (rp != OEA_OK) return rp;
    check_pairs_kernel<<<(unsigned)oea::ceil_div(n, 256), 256, 0, st>>>(pairs, n, n_str1, n_str2, err_flag);
    OEA_CHECK_HIP(hipGetLastError());
    const unsigned grid = (unsigned)std::min<int64_t>(n, kLcsGrid);
    lcs_pairs_kernel<<<grid, 64, 0, st>>>(p1, p2, pairs, n, lcs, ratio, workspace, max_len + 1, err_flag);
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

int oea_attr_sim_records(const int32_t *cp1, const int64_t *off1, int64_t n_str1, int64_t n_cp1, const int32_t *cp2, const int64_t *off2,
                         int64_t n_str2, int64_t n_cp2, int64_t max_len, int32_t K, const int32_t *idx1, int64_t n1,
                         const int32_t *idx2, int64_t n2, double threshold, const int32_t *rows, int64_t n_rows, int32_t cap,
                         int32_t *rec_col, double *rec_val, int32_t *rec_cnt, int32_t *overflow, int32_t *workspace, int32_t *err_flag,
                         void *stream) {
    const Pool p1{cp1, off1, n_str1, n_cp1}, p2{cp2, off2, n_str2, n_cp2};
    const int rc = check_pools(p1, p2, max_len);
    if (rc != OEA_OK) return rc;
    OEA_REQUIRE(K >= 1 && K <= kMaxK, "1 <= K <= 32 aligned attribute pairs");
    OEA_REQUIRE(n1 >= 1 && n2 >= 1 && n1 < ((int64_t)1 << 31) && n2 < ((int64_t)1 << 31), "1 <= n1, n2 < 2^31");
    OEA_REQUIRE(n_rows >= 0 && (rows || n_rows == n1), "rows == NULL takes n_rows == n1");
    OEA_REQUIRE(cap >= 1, "cap >= 1");
    OEA_REQUIRE(threshold == threshold, "threshold is NaN");
    OEA_REQUIRE(idx1 && idx2 && rec_col && rec_val && rec_cnt && overflow && workspace && err_flag, "null pointer");
    if (n_rows == 0) return OEA_OK;
    hipStream_t st = oea::as_stream(stream);
    const int rp = launch_pool_checks(p1, p2, max_len, err_flag, st);
    if (rp != OEA_OK) return rp;
    check_index_kernel<<<(unsigned)oea::ceil_div((int64_t)K * n1, 256), 256, 0, st>>>(idx1, (int64_t)K * n1, -1, n_str1, err_flag);
    OEA_CHECK_HIP(hipGetLastError());
    check_index_kernel<<<(unsigned)oea::ceil_div((int64_t)K * n2, 256), 256, 0, st>>>(idx2, (int64_t)K * n2, -1, n_str2, err_flag);
    OEA_CHECK_HIP(hipGetLastError());
    if (rows) {
        check_index_kernel<<<(unsigned)oea::ceil_div(n_rows, 256), 256, 0, st>>>(rows, n_rows, 0, n1, err_flag);
        OEA_CHECK_HIP(hipGetLastError());
    }
    RecArgs A;
    A.p1 = p1; A.p2 = p2; A.K = K; A.cap = cap;
    A.idx1 = idx1; A.idx2 = idx2; A.rows = rows;
    A.n1 = n1; A.n2 = n2; A.n_rows = n_rows;
    A.threshold = threshold;
    A.rec_col = rec_col; A.rec_cnt = rec_cnt; A.overflow = overflow; A.ws = workspace;
    A.rec_val = rec_val;
    A.ws_stride = max_len + 1;
    A.err = err_flag;
    const unsigned grid = (unsigned)std::min<int64_t>(n_rows, kLcsGrid);
    attr_sim_records_kernel<<<grid, 64 * kRecWaves, 0, st>>>(A);
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

}  // extern "C"
