// sample_distinct.hip -- m distinct draws from [0, n): random.sample(range(n), m) of the reference (attr2vec.py:150, jape.py:134).
//
// out[i] = pi(i), pi a keyed bijection of [0, n): a 6-round Feistel network over b = max(2, ceil(log2 n)) bits, split into a right
// half of b / 2 bits and a left half of b - b / 2, cycle-walked until the image is below n (the domain is < 2 n for n >= 2, so
// < 2 evaluations on average).  A Feistel network is a permutation of its domain whatever the round function is, and cycle
// walking restricts a permutation to a subset: the first m images are m distinct elements.  Round function: mix32(half ^ key);
// the six round keys are the words x, y, z, w of Philox4x32-10(counter = (step lo, step hi, 0x64697374, 0), key = (seed lo,
// seed hi)) and x, y of the same with counter word 3 = 1: a pure function of (seed, step), evaluated per element, no host read.
#include "common.h"

namespace {

constexpr uint32_t kTag = 0x64697374u;      // "dist"

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

__global__ void sample_distinct_kernel(uint32_t n, int64_t m, uint32_t k0, uint32_t k1, uint32_t s0, uint32_t s1, int lbits, int rbits,
                                       int32_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint4 wa = oea::philox4x32_10(s0, s1, kTag, 0u, k0, k1), wb = oea::philox4x32_10(s0, s1, kTag, 1u, k0, k1);
    const uint32_t key[6] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y};
    const uint32_t lmask = (1u << lbits) - 1u, rmask = (1u << rbits) - 1u;
    uint32_t x = (uint32_t)i;
    do {
        uint32_t l = x >> rbits, r = x & rmask;
#pragma unroll
        for (int q = 0; q < 6; q += 2) {
            l = (l ^ mix32(r ^ key[q])) & lmask;
            r = (r ^ mix32(l ^ key[q + 1])) & rmask;
        }
        x = (l << rbits) | r;
    } while (x >= n);
    out[i] = (int32_t)x;
}

}  // namespace

extern "C" {

int oea_sample_distinct(int64_t n, int64_t m, uint64_t seed, uint64_t step, int32_t *out, void *stream) {
    OEA_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "1 <= n < 2^31");
    OEA_REQUIRE(m >= 0 && m <= n, "0 <= m <= n");
    OEA_REQUIRE(out || m == 0, "null pointer");
    if (m == 0) return OEA_OK;
    int bits = 2;
    while (((int64_t)1 << bits) < n) ++bits;
    const int rbits = bits / 2, lbits = bits - rbits;
    sample_distinct_kernel<<<(unsigned)oea::ceil_div(m, 256), 256, 0, oea::as_stream(stream)>>>(
        (uint32_t)n, m, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)step, (uint32_t)(step >> 32), lbits, rbits, out);
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

}  // extern "C"
