// sim_tiles.h -- the MFMA tile pipelines of the similarity files (sim_rank.hip, topk.hip, csls_means.hip): 128 x 128 tiles of
// packed operands staged by LDS-DMA, in four forms -- fp32 (exact k-ordered chain), bf16 hi / lo split, the same on 256 x 128 tiles
// through a three-stage ring, and the split with the fixed operand in registers -- each a __device__ template that takes the
// caller's epilogue.  Below them, the host side every user shares: operand packing into the process-wide slots, the grid rules and
// the strip stores.  Their kernels, the slots and the switches exist once, in sim_rank.hip.
#pragma once
#include "common.h"

namespace oea {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TILE = 128;      // block tile edge (both operands)
constexpr int BK = 32;         // K chunk
constexpr int LDS_LD = BK + 4; // floats per row of an LDS chunk buffer (a packed chunk fills BK of them)

// ---- XCD-aware order of the (query tile, candidate chunk) work items (round 5) --------------------------------------------------
// Block b of a launch runs on XCD b % 8 (observed dispatch rule, MI355X_MICROARCH.md: "for speed only"), and every XCD has its own
// 4 MB L2.  In launch order (query tile fastest) the 64 workgroups resident on one XCD hold 64 DIFFERENT query tiles: from K = 300
// on their operand panels (128 rows x Kp x 4 B each, re-read once per candidate tile) no longer fit the L2 and every chunk comes
// from the Infinity Cache -- 185 GB per 70,000^2 x 1,200 sweep.  Here XCD c takes the contiguous share [c * per, (c + 1) * per) of
// the items in CHUNK-FASTEST order: its resident workgroups are ~64 / ny query tiles x all ny candidate chunks, i.e. 64 / ny + ny
// operand streams instead of 65, each k chunk fetched from the fabric once and hit in L2 by the other workgroups that walk the
// same panel in step.  per = 0: the plain order (OEA_XCD_MAP=0, ablation).  Correctness never depends on the placement.
struct TileGrid { unsigned nx, ny, per; };

__device__ __forceinline__ bool tile_grid_item(const TileGrid &g, unsigned &bx, unsigned &by) {
    const unsigned L = blockIdx.x;
    if (g.per == 0u) { bx = L % g.nx; by = L / g.nx; return L < g.nx * g.ny; }
    const unsigned slot = L >> 3, w = (L & 7u) * g.per + slot;
    if (slot >= g.per || w >= g.nx * g.ny) return false;
    bx = w / g.ny; by = w % g.ny;
    return true;
}

__device__ __forceinline__ uint32_t f2ord(float f) {   // order-preserving float -> uint
    uint32_t u = __float_as_uint(f + 0.0f);   // -0 -> +0 so that key order == float order
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o); }

__device__ __forceinline__ void zero_acc(f32x16 (&acc)[2][2]) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
}

// ---- packed operands + LDS-DMA staging --------------------------------------------------------------------------
// A chunk goes HBM/L2 -> LDS by `global_load_lds_dwordx4` (gfx950) without passing through registers and without
// ds_write instructions.  The LDS-DMA destination of one wave instruction is lane-linear (base + 16 B * lane), so the k
// permutation cannot be applied on the way: the operands are packed once per call by pack_rows_kernel ([n_pad, Kp] with
// n_pad % 128 == 0 and Kp % 32 == 0, zero filled, every group of 8 k stored as k = 0,2,4,6,1,3,5,7 -- O(n d) work in
// front of an O(n^2 d) sweep).  The LDS image of a chunk is 128 rows x 32 floats WITHOUT padding; bank conflicts are
// avoided by an XOR swizzle of the eight 16-byte columns of a row with ((row >> 1) & 7), applied to the per-lane SOURCE
// address of the DMA and to the ds_read address (the same involution on both sides).  A 128-byte row covers half of the
// 64 banks, so 16 consecutive rows of one column must land on all 16 (row parity, position) combinations: with
// (row & 7) rows r and r + 8 collided -- SQ_LDS_BANK_CONFLICT was half of SQ_LDS_IDX_ACTIVE -- with ((row >> 1) & 7)
// they do not.
constexpr int PLD = BK;                 // unpadded LDS row stride (floats)

// rows [row0, row0 + 128) x packed k [k0, k0 + 32) -> LDS buffer `dst` (128 x 32 floats), 4 DMA instructions per wave
__device__ __forceinline__ void stage_packed(const float *__restrict__ packed, int kp, int64_t row0, int k0,
                                             float *__restrict__ dst) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane >> 3;                                         // row inside the instruction's 8-row block
    const float *src = packed + (row0 + wave * 32 + sub) * kp + k0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float *base = dst + (wave * 4 + j) * 8 * PLD;                  // wave-uniform: 1 KB per instruction
        const int swz = (4 * j + (sub >> 1)) & 7;                      // ((row >> 1) & 7) of row = 32 wave + 8 j + sub
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + (int64_t)j * 8 * kp + 4 * ((lane & 7) ^ swz)),
                                         reinterpret_cast<__attribute__((address_space(3))) void *>(reinterpret_cast<uintptr_t>(base)),
                                         16, 0, 0);
    }
}

__device__ __forceinline__ void mma_chunk_packed(const float *__restrict__ As, const float *__restrict__ Bs, int groups,
                                                 f32x16 (&acc)[2][2]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int x = (lane >> 1) & 7, half = lane >> 5;                   // ((row >> 1) & 7): tile offsets are multiples of 16
    const float *ap = As + (wm * 64 + (lane & 31)) * PLD;
    const float *bp = Bs + (wn * 64 + (lane & 31)) * PLD;
    for (int g = 0; g < groups; ++g) {
        const int off = 4 * ((2 * g + half) ^ x);
        const float4 a0 = *reinterpret_cast<const float4 *>(ap + off);
        const float4 a1 = *reinterpret_cast<const float4 *>(ap + 32 * PLD + off);
        const float4 b0 = *reinterpret_cast<const float4 *>(bp + off);
        const float4 b1 = *reinterpret_cast<const float4 *>(bp + 32 * PLD + off);
        const float av[2][4] = {{a0.x, a0.y, a0.z, a0.w}, {a1.x, a1.y, a1.z, a1.w}};
        const float bv[2][4] = {{b0.x, b0.y, b0.z, b0.w}, {b1.x, b1.y, b1.z, b1.w}};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[0][s], bv[0][s], acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[0][s], bv[1][s], acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[1][s], bv[0][s], acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[1][s], bv[1][s], acc[1][1], 0, 0, 0);
        }
    }
}

// Software pipeline over a sequence of `n_tiles` M-tiles against one fixed N-tile on packed operands (am / bn: packed
// arrays, Kp floats per row; rows are padded, so no clamping): the DMA of chunk i+1 is issued into the other LDS buffer
// before chunk i goes to the matrix cores; the barrier at the end of the iteration (with the vmcnt(0) the compiler puts in
// front of it) makes it visible and frees the buffer just read.  `epilogue(t, acc)` runs after the last chunk of M-tile t.
// LDS: As/Bs = 2 buffers of TILE*LDS_LD floats each.  The fp32 tile kernels receive the packed operands and their Kp in the
// (table, ld) arguments.
template <class MTile, class Epilogue>
__device__ __forceinline__ void tile_pipeline_packed(const float *__restrict__ am, int kp, const float *__restrict__ bn,
                                                     int dim, int64_t n0, int64_t n_tiles, MTile m_tile, float *As,
                                                     float *Bs, Epilogue epilogue) {
    const int kend = (dim + 7) / 8 * 8;
    const int nchunk = (kend + BK - 1) / BK;
    const int64_t total = n_tiles * nchunk;
    if (total == 0) return;
    constexpr int BUF = TILE * LDS_LD;
    stage_packed(am, kp, m_tile(0), 0, As);
    stage_packed(bn, kp, n0, 0, Bs);
    __syncthreads();
    f32x16 acc[2][2];
    zero_acc(acc);
    int64_t t = 0;
    int kc = 0;
    for (int64_t it = 0; it < total; ++it) {
        const int cur = (int)(it & 1);
        if (it + 1 < total) {
            int kc1 = kc + 1;
            int64_t t1 = t;
            if (kc1 == nchunk) { kc1 = 0; ++t1; }
            stage_packed(am, kp, m_tile(t1), kc1 * BK, As + (cur ^ 1) * BUF);
            stage_packed(bn, kp, n0, kc1 * BK, Bs + (cur ^ 1) * BUF);
        }
        mma_chunk_packed(As + cur * BUF, Bs + cur * BUF, min(BK, kend - kc * BK) / 8, acc);
        __syncthreads();
        if (++kc == nchunk) {
            epilogue(t, acc);
            zero_acc(acc);
            kc = 0;
            ++t;
        }
    }
}

// ---- bf16 hi / lo split operands (certified prefilter: see rank_bf16_kernel, sim_rank.hip) -------------------------------------
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;

__device__ __forceinline__ uint32_t bf16_rne(float x) {                   // round to nearest even (finite inputs)
    const uint32_t u = __float_as_uint(x);
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

// acc += hi.hi + hi.lo + lo.hi of one chunk (ksteps = 1 or 2 k-steps of 16)
// EARLY (the 256 x 128 kernels): all eight fragment reads of a k-step are issued in front of its MFMAs (a scheduling fence keeps
// them there) in the order the products consume them, so the waits are counted lgkmcnt(6 / 4 / 2 / 0) behind running MFMAs; left
// to itself hipcc re-uses the hi fragments' registers for the lo ones and waits for the LDS with lgkmcnt(0) three times per k-step
template <bool EARLY = false>
__device__ __forceinline__ void mma_chunk_bf16(const float *__restrict__ As, const float *__restrict__ Bs, int ksteps,
                                               f32x16 (&acc)[2][2]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int x = (lane >> 1) & 7, half = lane >> 5;
    const float *ap = As + (wm * 64 + (lane & 31)) * PLD;
    const float *bp = Bs + (wn * 64 + (lane & 31)) * PLD;
    for (int s = 0; s < ksteps; ++s) {
        const int g = 4 * s + 2 * half;
        const int oh = 4 * (g ^ x), ol = 4 * ((g + 1) ^ x);
        const bf16x8 a0h = *reinterpret_cast<const bf16x8 *>(ap + oh), b0h = *reinterpret_cast<const bf16x8 *>(bp + oh);
        const bf16x8 b1h = *reinterpret_cast<const bf16x8 *>(bp + 32 * PLD + oh), a1h = *reinterpret_cast<const bf16x8 *>(ap + 32 * PLD + oh);
        const bf16x8 b0l = *reinterpret_cast<const bf16x8 *>(bp + ol), b1l = *reinterpret_cast<const bf16x8 *>(bp + 32 * PLD + ol);
        const bf16x8 a0l = *reinterpret_cast<const bf16x8 *>(ap + ol), a1l = *reinterpret_cast<const bf16x8 *>(ap + 32 * PLD + ol);
        if constexpr (EARLY) __builtin_amdgcn_sched_barrier(0);
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0h, b0h, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0h, b1h, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1h, b0h, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1h, b1h, acc[1][1], 0, 0, 0);
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0h, b0l, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0h, b1l, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1h, b0l, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1h, b1l, acc[1][1], 0, 0, 0);
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0l, b0h, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0l, b1h, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1l, b0h, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1l, b1h, acc[1][1], 0, 0, 0);
    }
}

// tile_pipeline_packed for the bf16 layout: chunks of two k-steps (32 k = 128 B per row), LDS-DMA staging unchanged.
// K BLOCKS (round 5; KBLK: the evaluation / CSLS sweeps -- the neighbour sweeps' epilogues have no 64 registers to spare and run at
// K = 100): the MFMA accumulators restart from zero every kBf16BlockChunks chunks (128 k) and
// the block results are added in block order on the VALU (64 v_add per 96 MFMAs).  The accumulation term of the certificate
// (bf16_eps_rel) then counts the products of ONE block: the error of n additions in any order is <= n u (sum of |terms|), and the
// blocks' sums of |terms| add up to <= |q||c| (Cauchy-Schwarz per block, then over the blocks) -- 3 * 128 + (blocks - 1)
// roundings instead of 3 * Kp: at K = 1,200 the bound drops from 5.9e-4 to 1.3e-4 and with it the records per row.
constexpr int kBf16BlockChunks = 4;

__device__ __forceinline__ void add_acc(f32x16 (&tot)[2][2], const f32x16 (&acc)[2][2]) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) tot[a][b][r] += acc[a][b][r];
}

template <bool KBLK, class MTile, class Epilogue>
__device__ __forceinline__ void tile_pipeline_bf16(const float *__restrict__ am, int kp, const float *__restrict__ bn, int dim,
                                                   int64_t n0, int64_t n_tiles, MTile m_tile, float *As, float *Bs,
                                                   Epilogue epilogue) {
    const int S = (dim + 15) / 16;
    const int nchunk = (S + 1) / 2;
    const int64_t total = n_tiles * nchunk;
    if (total == 0) return;
    constexpr int BUF = TILE * LDS_LD;
    stage_packed(am, kp, m_tile(0), 0, As);
    stage_packed(bn, kp, n0, 0, Bs);
    __syncthreads();
    f32x16 acc[2][2], tot[2][2];
    zero_acc(acc);
    zero_acc(tot);
    int64_t t = 0;
    int kc = 0;
    for (int64_t it = 0; it < total; ++it) {
        const int cur = (int)(it & 1);
        if (it + 1 < total) {
            int kc1 = kc + 1;
            int64_t t1 = t;
            if (kc1 == nchunk) { kc1 = 0; ++t1; }
            stage_packed(am, kp, m_tile(t1), kc1 * BK, As + (cur ^ 1) * BUF);
            stage_packed(bn, kp, n0, kc1 * BK, Bs + (cur ^ 1) * BUF);
        }
        mma_chunk_bf16(As + cur * BUF, Bs + cur * BUF, min(2, S - 2 * kc), acc);
        ++kc;
        if constexpr (KBLK) {
            if ((kc & (kBf16BlockChunks - 1)) == 0 || kc == nchunk) {   // end of a 128-k block: block sums in block order (one
                add_acc(tot, acc);                                      // block when K <= 128: tot = 0 + acc, the same values)
                zero_acc(acc);
            }
        }
        // the epilogue works on registers only: it runs BEFORE the barrier (and the vmcnt(0) in front of it), so the DMA of the
        // next tile's first chunk lands behind it instead of being waited for first (the bf16 chunks are too short to hide it)
        if (kc == nchunk) {
            if constexpr (KBLK) { epilogue(t, tot); zero_acc(tot); }
            else { epilogue(t, acc); zero_acc(acc); }
            kc = 0;
            ++t;
        }
        __syncthreads();
    }
}

// ---- 256 x 128 tiles, three LDS stages (round 5: K > 128, i.e. AliNet's 1,200-d / RDGCN's 300-d evaluation rows) ---------------
// tile_pipeline_bf16 keeps ONE 32 KB chunk per workgroup in flight (64 KB per CU): with ~1.9 us between the issue of a chunk's
// LDS-DMA and its arrival under load that is 34 GB/s per CU -- the 70,000^2 x 1,200 sweep sat at 34 % of the bf16 pipe whatever
// the epilogue did.  Here 512 threads (8 waves as 4 (M) x 2 (N), each still a 64 x 64 sub-tile: every epilogue is unchanged) own
// 256 candidate rows x 128 query rows -- 3/4 of the operand bytes per flop -- and a ring of THREE 48 KB stages keeps TWO chunks in
// flight (96 KB per CU): a chunk is waited for with a COUNTED s_waitcnt vmcnt(6) (6 DMA instructions per wave and stage: the
// newer stage stays in flight) in front of a RAW s_barrier -- __syncthreads() would drain the DMA queue (vmcnt(0)) on every chunk.
// K blocks as in tile_pipeline_bf16<true>.  LDS: 3 x (256 + 128) x 128 B = 144 KB (dynamic), one workgroup per CU.
constexpr int BIG_MT = 256;                       // candidate rows of a tile
constexpr int BIG_A = BIG_MT * PLD;               // floats of an A stage
constexpr int BIG_STAGE = BIG_A + TILE * PLD;     // + the B stage: 48 KB
constexpr int BIG_STAGES = 3;
constexpr int BIG_LDS_BYTES = BIG_STAGES * BIG_STAGE * 4;

// per-lane part of the DMA source addresses of a stage (elements): the swizzled 16-byte column of the lane's row for the even /
// odd 8-row pieces; everything else of an address is wave-uniform (tile row, k chunk, piece) and stays on the scalar unit
struct BigLane {
    unsigned a_even, a_odd, b_even, b_odd;
    float *a_dst, *b_dst;                 // LDS offsets of the wave's pieces inside a stage
};

__device__ __forceinline__ BigLane big_lane(int kp) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;          // 8 waves: 32 A rows + 16 B rows each
    const int sub = lane >> 3;
    BigLane l;
    const unsigned c_even = 4u * ((lane & 7) ^ ((sub >> 1) & 7)), c_odd = 4u * ((lane & 7) ^ ((4 + (sub >> 1)) & 7));   // ((row >> 1) & 7), row = 8 j + sub (+ 16 or 32 wave)
    l.a_even = (unsigned)(wave * 32 + sub) * (unsigned)kp + c_even;
    l.a_odd = (unsigned)(wave * 32 + sub) * (unsigned)kp + c_odd;
    l.b_even = (unsigned)(wave * 16 + sub) * (unsigned)kp + c_even;
    l.b_odd = (unsigned)(wave * 16 + sub) * (unsigned)kp + c_odd;
    l.a_dst = nullptr; l.b_dst = nullptr;
    return l;
}

__device__ __forceinline__ void stage_packed_big(const float *__restrict__ a_tile /* am + row0 * kp + k0: wave-uniform */,
                                                 const float *__restrict__ b_tile, int kp, const BigLane &l, float *__restrict__ slot) {
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float *base = slot + (wave * 4 + j) * 8 * PLD;
        const float *src = a_tile + (size_t)((j & 1 ? l.a_odd : l.a_even) + (unsigned)(j * 8 * kp));
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                         reinterpret_cast<__attribute__((address_space(3))) void *>(reinterpret_cast<uintptr_t>(base)),
                                         16, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        float *base = slot + BIG_A + (wave * 2 + j) * 8 * PLD;
        const float *src = b_tile + (size_t)((j & 1 ? l.b_odd : l.b_even) + (unsigned)(j * 8 * kp));
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                         reinterpret_cast<__attribute__((address_space(3))) void *>(reinterpret_cast<uintptr_t>(base)),
                                         16, 0, 0);
    }
}

// the eight fragments of one k-step of a wave's 64 x 64 sub-tile
struct BfFrag { bf16x8 a0h, a0l, a1h, a1l, b0h, b0l, b1h, b1l; };

__device__ __forceinline__ void load_bf_frag(const float *__restrict__ ap, const float *__restrict__ bp, int s, int half, int x, BfFrag &f) {
    const int g = 4 * s + 2 * half;
    const int oh = 4 * (g ^ x), ol = 4 * ((g + 1) ^ x);
    f.a0h = *reinterpret_cast<const bf16x8 *>(ap + oh); f.b0h = *reinterpret_cast<const bf16x8 *>(bp + oh);
    f.b1h = *reinterpret_cast<const bf16x8 *>(bp + 32 * PLD + oh); f.a1h = *reinterpret_cast<const bf16x8 *>(ap + 32 * PLD + oh);
    f.b0l = *reinterpret_cast<const bf16x8 *>(bp + ol); f.b1l = *reinterpret_cast<const bf16x8 *>(bp + 32 * PLD + ol);
    f.a0l = *reinterpret_cast<const bf16x8 *>(ap + ol); f.a1l = *reinterpret_cast<const bf16x8 *>(ap + 32 * PLD + ol);
}

__device__ __forceinline__ void mma_bf_frag(const BfFrag &f, f32x16 (&acc)[2][2]) {
    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a0h, f.b0h, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a0h, f.b1h, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a1h, f.b0h, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a1h, f.b1h, acc[1][1], 0, 0, 0);
    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a0h, f.b0l, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a0h, f.b1l, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a1h, f.b0l, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a1h, f.b1l, acc[1][1], 0, 0, 0);
    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a0l, f.b0h, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a0l, f.b1h, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a1l, f.b0h, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a1l, f.b1h, acc[1][1], 0, 0, 0);
}

// PF (the plain sweeps): the fragment reads never wait in front of idle matrix cores.  A chunk is two k-steps; the loop
// body is  [reads of k-step 1 of chunk c] [MFMAs of k-step 0] [chunk c + 1 landed? counted vmcnt, raw barrier] [DMA of chunk c + 3 into
// the slot chunk c just left] [reads of k-step 0 of chunk c + 1] [MFMAs of k-step 1 of chunk c]: every read is issued one MFMA group
// (12 x 32 cycles) before its use, the barrier sits between the two groups, and the DMA runs three chunks ahead.  The second k-step of
// a tile's last chunk may be zero padding of the packed rows (Kp is a multiple of 32): it adds +0.  !PF = the first form of this
// pipeline (reads in front of each group, barrier at the top): the sweep with the CSLS terms in its epilogue, where PF spills.
template <bool PF, class MTile, class Epilogue>
__device__ __forceinline__ void tile_pipeline_bf16_big(const float *__restrict__ am, int kp, const float *__restrict__ bn, int dim,
                                                       int64_t n0, int64_t n_tiles, MTile m_tile, float *lds, Epilogue epilogue) {
    const int S = (dim + 15) / 16;
    const int nchunk = (S + 1) / 2;
    const int total = (int)n_tiles * nchunk;          // (a work item walks at most a few thousand chunks)
    if (total <= 0) return;
    const BigLane lane_off = big_lane(kp);
    const float *b_base = bn + n0 * kp;
    int ti = 0, ki = 0, si = 0;                       // (tile, chunk, LDS stage) of the next stage to issue
    const float *a_base = am + m_tile(0) * kp;
    auto issue = [&]() {
        stage_packed_big(a_base + ki * BK, b_base + ki * BK, kp, lane_off, lds + si * BIG_STAGE);
        si = si == BIG_STAGES - 1 ? 0 : si + 1;
        if (++ki == nchunk) { ki = 0; ++ti; a_base = am + m_tile(ti) * kp; }
    };
    f32x16 acc[2][2], tot[2][2];
    zero_acc(acc);
    zero_acc(tot);
    int t = 0, kc = 0, sc = 0;                        // (tile, chunk, stage) being multiplied
    if constexpr (!PF) {
        issue();
        if (total > 1) issue();
        for (int it = 0; it < total; ++it) {
            // stage `it` has landed when at most the newer stage's 6 DMA instructions of this wave are outstanding (loads complete in
            // order; whatever the epilogue issued since only makes the count stricter); the barrier then covers the other waves' parts
            // and tells everybody that the slot read in iteration it - 1 is free
            if (it + 1 < total) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            if (it + 2 < total) issue();
            const float *slot = lds + sc * BIG_STAGE;
            sc = sc == BIG_STAGES - 1 ? 0 : sc + 1;
            mma_chunk_bf16<true>(slot, slot + BIG_A, min(2, S - 2 * kc), acc);
            ++kc;
            if ((kc & (kBf16BlockChunks - 1)) == 0 || kc == nchunk) {
                add_acc(tot, acc);
                zero_acc(acc);
            }
            if (kc == nchunk) {
                epilogue((int64_t)t, tot);
                zero_acc(tot);
                kc = 0;
                ++t;
            }
        }
        return;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int x = (lane >> 1) & 7, half = lane >> 5;
    const int a_off = (wm * 64 + (lane & 31)) * PLD, b_off = BIG_A + (wn * 64 + (lane & 31)) * PLD;
    // prologue: three chunks on their way, chunk 0 landed, its first fragments requested
    issue();
    if (total > 1) issue();
    if (total > 2) issue();
    if (total > 2) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else if (total > 1) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    BfFrag f0, f1;
    load_bf_frag(lds + a_off, lds + b_off, 0, half, x, f0);
    for (int it = 0; it < total; ++it) {
        const float *slot = lds + sc * BIG_STAGE;
        load_bf_frag(slot + a_off, slot + b_off, 1, half, x, f1);            // k-step 1 of this chunk, behind the MFMAs of k-step 0
        __builtin_amdgcn_sched_barrier(0);
        mma_bf_frag(f0, acc);
        __builtin_amdgcn_sched_barrier(0);
        sc = sc == BIG_STAGES - 1 ? 0 : sc + 1;
        if (it + 1 < total) {
            // chunk it + 1 must have landed: of this wave's DMA only chunk it + 2's (6 instructions) may still be out; f1 has arrived
            // too (lgkmcnt(0)): after the barrier nobody reads chunk it's slot any more
            if (it + 2 < total) asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            if (it + 3 < total) issue();                                     // into the slot of chunk it
            const float *nxt = lds + sc * BIG_STAGE;
            load_bf_frag(nxt + a_off, nxt + b_off, 0, half, x, f0);          // k-step 0 of the next chunk, behind the MFMAs of k-step 1
        }
        __builtin_amdgcn_sched_barrier(0);
        mma_bf_frag(f1, acc);
        __builtin_amdgcn_sched_barrier(0);
        ++kc;
        if ((kc & (kBf16BlockChunks - 1)) == 0 || kc == nchunk) {
            add_acc(tot, acc);
            zero_acc(acc);
        }
        if (kc == nchunk) {
            epilogue((int64_t)t, tot);
            zero_acc(tot);
            kc = 0;
            ++t;
        }
    }
}

// B IN REGISTERS (round 4, Kp = 32 NCH <= 128).  tile_pipeline_bf16 stages a 16 KB chunk of BOTH operands per iteration and waits for
// it at the next barrier: with the matrix part of a chunk down to ~700 cycles the L2 / fabric latency of the chunk (~2 us) is what
// an iteration takes -- the bf16 pipeline alone ran at 15 % of the matrix pipe.  The B tile of a work item never changes: here every
// lane loads its B fragments of ALL k-steps once, straight from the packed rows into registers (32 NCH VGPRs), the LDS holds only A
// stages, and a stage is TWO chunks (32 KB): half the barriers and exposed latencies per tile, half the LDS reads, no B re-reads.
// As: 2 slots x 2 chunks x (128 x 32) floats = 64 KB.
template <int NCH>
struct BRegs {
    bf16x8 h[2 * NCH][2], l[2 * NCH][2];             // [k-step][row block tn]: hi and lo fragments of this lane
};

template <int NCH>
__device__ __forceinline__ void load_bregs(const float *__restrict__ bn, int kp, int64_t n0, BRegs<NCH> &b) {
    const int lane = threadIdx.x & 63, wave = (threadIdx.x >> 6) & 3;
    const int wn = wave & 1, half = lane >> 5;
    const float *row = bn + (n0 + wn * 64 + (lane & 31)) * kp + half * 8;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int tn = 0; tn < 2; ++tn) {
                const float *p = row + (int64_t)tn * 32 * kp + c * 32 + s2 * 16;     // granules ((s2 * 2 + half) * 2 + {0, 1}) of chunk c
                b.h[2 * c + s2][tn] = *reinterpret_cast<const bf16x8 *>(p);
                b.l[2 * c + s2][tn] = *reinterpret_cast<const bf16x8 *>(p + 4);
            }
}

// acc += the three split products of chunk c (two k-steps): A fragments from the staged chunk, B fragments from registers
// one_step: only the chunk's first k-step (the second one is the zero padding of a row whose 16-k steps are odd in number: dim = 100 is
// seven steps -- an eighth of the tile's MFMAs and fragment reads)
template <int NCH>
__device__ __forceinline__ void mma_chunk_breg(const float *__restrict__ As, const BRegs<NCH> &b, int c, f32x16 (&acc)[2][2], bool one_step = false) {
    const int lane = threadIdx.x & 63, wave = (threadIdx.x >> 6) & 3;
    const int wm = wave >> 1;
    const int x = (lane >> 1) & 7, half = lane >> 5;
    const float *ap = As + (wm * 64 + (lane & 31)) * PLD;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
        if (s2 == 1 && one_step) break;                               // wave-uniform
        const int g = 4 * s2 + 2 * half;
        const int oh = 4 * (g ^ x), ol = 4 * ((g + 1) ^ x);
        const bf16x8 a0h = *reinterpret_cast<const bf16x8 *>(ap + oh), a0l = *reinterpret_cast<const bf16x8 *>(ap + ol);
        const bf16x8 a1h = *reinterpret_cast<const bf16x8 *>(ap + 32 * PLD + oh), a1l = *reinterpret_cast<const bf16x8 *>(ap + 32 * PLD + ol);
        const bf16x8 b0h = b.h[2 * c + s2][0], b0l = b.l[2 * c + s2][0], b1h = b.h[2 * c + s2][1], b1l = b.l[2 * c + s2][1];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0h, b0h, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0h, b1h, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1h, b0h, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1h, b1h, acc[1][1], 0, 0, 0);
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0h, b0l, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0h, b1l, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1h, b0l, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1h, b1l, acc[1][1], 0, 0, 0);
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0l, b0h, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0l, b1h, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1l, b0h, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1l, b1h, acc[1][1], 0, 0, 0);
    }
}

template <int NCH, class MTile, class Epilogue>
__device__ __forceinline__ void tile_pipeline_bf16_breg(const float *__restrict__ am, int kp, const float *__restrict__ bn, int64_t n0,
                                                        int64_t n_tiles, MTile m_tile, float *As, Epilogue epilogue, int dim = 0) {
    constexpr int BUF = TILE * PLD;                                   // one chunk
    constexpr int NS = (NCH + 1) / 2;                                 // stages per tile: chunks [2 s, min(2 s + 2, NCH))
    const int64_t total = n_tiles * NS;
    if (total == 0) return;
    const bool odd_steps = dim > 0 && (dim + 15) / 16 == 2 * NCH - 1; // the last chunk's second k-step is padding
    BRegs<NCH> b;
    load_bregs<NCH>(bn, kp, n0, b);
    auto stage = [&](int64_t t, int s, float *slot) {
        stage_packed(am, kp, m_tile(t), (2 * s) * BK, slot);
        if (2 * s + 1 < NCH) stage_packed(am, kp, m_tile(t), (2 * s + 1) * BK, slot + BUF);
    };
    stage(0, 0, As);
    __syncthreads();
    f32x16 acc[2][2];
    zero_acc(acc);
    int64_t t = 0;
    int sidx = 0;
    for (int64_t it = 0; it < total; ++it) {
        float *cur = As + (it & 1) * 2 * BUF, *nxt = As + ((it & 1) ^ 1) * 2 * BUF;
        if (it + 1 < total) {
            int s1 = sidx + 1;
            int64_t t1 = t;
            if (s1 == NS) { s1 = 0; ++t1; }
            stage(t1, s1, nxt);
        }
#pragma unroll
        for (int s = 0; s < NS; ++s)                                 // (compile-time chunk indices for the register file)
            if (s == sidx) {
                mma_chunk_breg<NCH>(cur, b, 2 * s, acc, odd_steps && 2 * s == NCH - 1);
                if (2 * s + 1 < NCH) mma_chunk_breg<NCH>(cur + BUF, b, 2 * s + 1, acc, odd_steps && 2 * s + 1 == NCH - 1);
            }
        if (++sidx == NS) {                                          // before the barrier: see tile_pipeline_bf16
            epilogue(t, acc);
            zero_acc(acc);
            sidx = 0;
            ++t;
        }
        __syncthreads();
    }
}

// ---- host side (defined in sim_rank.hip unless noted) --------------------------------------------------------------------------
struct PackedOp {
    float *p = nullptr;      // [n_pad, kp] in the process-wide scratch slot
    int kp = 0;
};

// Operand slots: 0 = queries, 1 = candidates, 2 / 3 = column / row samples (neighbour search, CSLS means), 3 also = the bf16 split
// rows of the neighbour search, 4 / 5 = the bf16 split operands of the CSLS means and of the neighbour search's candidates.
// pack_operand: the fp32 layout of pack_rows_kernel; pack_operand_bf16: the hi / lo split; reserve_operand: the slot's buffer
// without a pack launch (the caller fills it, or finds there what an earlier pack of this call left).  release_packed after the
// kernels that read the packed operands have been enqueued.
int pack_operand(int slot, const float *src, int64_t n, int ld, int dim, hipStream_t st, PackedOp *out);
int pack_operand_bf16(int slot, const float *src, int64_t n, int ld, int dim, hipStream_t st, PackedOp *out);
int reserve_operand(int slot, int64_t n, int dim, hipStream_t st, PackedOp *out, int64_t *n_pad_out);
int release_packed(hipStream_t st);

// candidate chunks per query tile so that the grid fills the chip (OEA_RANK_WGS); the XCD-aware item order (OEA_XCD_MAP)
int pick_chunks(int64_t q_tiles, int64_t c_tiles, int *tiles_per_chunk);
TileGrid make_tile_grid(unsigned nx, unsigned ny);
unsigned tile_grid_blocks(const TileGrid &g);

// relative bound on |v~ - v| of a bf16 split sweep, in units of |q| |c|; k_blocks: tile_pipeline_bf16<true> / _big
float bf16_eps_rel(int dim, bool k_blocks);
// tol_dev[0] = that bound for the tables a and b (b == NULL: a against itself) from their largest row norms, which land in
// tol_dev[1] and tol_dev[2] (b only); the caller has zeroed those
void bf16_tol_bound(const float *a, int64_t na, int lda, const float *b, int64_t nb, int ldb, int dim, bool k_blocks, float *tol_dev,
                    hipStream_t st);

// strips of S from packed operands: out[n1, ld_out] = e1p e2p^T, exact fp32 chain; gate != NULL: nothing is computed when *gate == 0
void sim_inner_store_packed(const float *e1p, int64_t n1, const float *e2p, int64_t n2, int kp, int dim, float *out, int64_t ld_out,
                            hipStream_t st, const int32_t *gate = nullptr);
// the same on the bf16 split (approximate: sampled thresholds are estimates).  _pack: the query rows into slot 3 (the sweep that
// follows finds them there) and every stride-th candidate row into slot 2
int sample_strip_bf16_pack(const float *q, int64_t nq, int ldq, const float *c, int64_t n_sample, int ld_sample, int dim, hipStream_t st,
                           const float **qs, const float **ss, int *kp);
void sample_strip_bf16_launch(const float *qs, int64_t rows, const float *ss, int64_t n_sample, int kp, int dim, float *strip, hipStream_t st);

// topk.hip: r-th largest of every row of a sample strip; gather of <= 128 listed packed rows (the fallbacks of the CSLS means)
int kth_value(const float *strip, int64_t rows, int sample, int r, float *thr, hipStream_t st);
void gather_packed_rows(const float *qp, int kp, const int32_t *rows, const int32_t *n_rows, float *dst, hipStream_t st);

}  // namespace oea
