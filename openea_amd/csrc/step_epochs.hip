// step_epochs.hip -- everything above ONE translational step, for gfx950: the batches of an epoch enqueued by one call, on one GPU
// or partitioned over G ranks.
//
//   oea_triple_epoch_range        one GPU: the epoch's negatives drawn ahead, the gathered-sum plan (step_plan.h) where
//                                 oea_step_plan_supported admits it, then the steps, each through oea::step_phase_planned;
//   oea_triple_epoch_range_comm   G ranks under the entity-id partition, dense protocol: part_pack / part_apply / part_unpack
//                                 around a reduce-scatter and an all-gather (also step by step from the host: oea_part_*);
//   oea_triple_epoch_range_halo   the same partition exchanging only the rows a step refers to (halo_*; oea_halo_plan shows the
//                                 row lists alone).
// All three are ONE walk over the batches (EpochWalk, epoch_walk).  The step itself lives in triple_step.hip and is called through
// the C entry points (oea_triple_step_phase, oea_step_apply_normals) and oea::step_phase_planned; what both units share -- the
// workspace, the row fragments, apply_one_row, the width ladders, the counts of loss partials -- is step_rows.h.  The optimiser
// kernels here (part_apply_kernel, halo_apply_kernel) take their group width from for_apply_width, the single-GPU job's rule, so a
// G-rank job of the fixed-point build equals the single-GPU job bit for bit.
#include <algorithm>
#include <vector>

#include "common.h"
#include "step_plan.h"
#include "step_rows.h"

namespace {

// ---- entity-id partitioning of the step (one process per GPU; BASELINE.json north_star) -----------------------
// Owner of entity row id = id mod G (ids are degree-ordered with the two KGs interleaved, read.py:64-79: contiguous ranges
// would put every hub on rank 0).  Every rank keeps a full READ copy of the table for its gathers and the optimiser state
// of its own rows only.  Per step:
//   GRAD phase (unchanged kernels)        -> local gradient scratch
//   part_pack_kernel                      -> send buffer in OWNER-MAJOR order [G][rpr * (ld + 1)] (rows then touched flags),
//                                            scratch rows + flags cleared on the way; relation rows to a small buffer
//   reduce-scatter (RCCL)                 -> this rank's rows summed over the ranks [rpr * (ld + 1)]
//   all-reduce of the relation buffer     (a few hundred rows: replicated, every rank applies the same update)
//   part_apply_kernel                     -> optimiser on the owned rows (strided in the natural table), updated rows also
//                                            written to a contiguous block for the all-gather; relation rows
//   all-gather (RCCL)                     -> everyone's updated rows [G][rpr][ld]
//   part_unpack_kernel                    -> the other ranks' rows into the local read copy
// The collectives move (G-1)/G * E * (2 ld + 1) * 4 bytes per rank and step -- the volume of the all-reduce they replace --
// but the optimiser runs on 1/G of the rows and its state is sharded.
template <int G, int IT>
__global__ __launch_bounds__(256) void part_pack_kernel(StepWs ws, int64_t n_ent, int64_t n_rel, int ld, int world, int64_t rpr,
                                                        grad_t *__restrict__ send, grad_t *__restrict__ rel_x) {
    const int lane = threadIdx.x % G;
    const int64_t grp = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int64_t ngrp = (int64_t)gridDim.x * blockDim.x / G;
    const int64_t chunk = rpr * (ld + 1);
    const int64_t slots = (int64_t)world * rpr;
    for (int64_t w = grp; w < slots + n_rel; w += ngrp) {
        if (w >= slots) {                                          // relation row: grads (copies folded by the GRAD phase) + flag
            const int64_t r = w - slots;
            const flag_t f = ws.rel_touched[r];
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                const int c = it * G + lane;
                if (c < ld) {
                    rel_x[r * ld + c] = f != 0 ? ws.rel_grad[r * ld + c] : (grad_t)0;
                    if (f != 0) ws.rel_grad[r * ld + c] = 0;
                }
            }
            if (lane == 0) { rel_x[n_rel * ld + r] = f; ws.rel_touched[r] = 0; }
            continue;
        }
        const int64_t o = w / rpr, j = w - o * rpr, id = j * world + o;        // slot (o, j) holds entity id
        const flag_t f = id < n_ent ? ws.ent_touched[id] : (flag_t)0;
        grad_t *dst = send + o * chunk + j * ld;
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int c = it * G + lane;
            if (c < ld) {
                dst[c] = f != 0 ? ws.ent_grad[id * ld + c] : (grad_t)0;
                if (f != 0) ws.ent_grad[id * ld + c] = 0;
            }
        }
        if (lane == 0) {
            send[o * chunk + rpr * ld + j] = f;
            if (f != 0) ws.ent_touched[id] = 0;
        }
    }
}

// one relation row of the partitioned jobs: its gradient is the row of rel_x (summed over the ranks), its flag follows rel_x's rows
// (rv, rg, ra: the caller's fragments, which its entity rows use next.  With fragments of its own the kernels take more registers:
//  part_apply_kernel<64, 8> 62 -> 69 VGPRs, 8 -> 7 waves per SIMD)
template <int G, int IT>
__device__ __forceinline__ void apply_exchanged_relation_row(int64_t r, float *rel, float *rel_acc, int64_t n_rel, int ld, int lane,
                                                             grad_t *rel_x, const oea_step_cfg &cfg, Row<G, IT> &rv, Row<G, IT> &rg,
                                                             Row<G, IT> &ra) {
    if (rel_x[n_rel * ld + r] == 0) return;
    rv.load(rel + r * ld, ld, lane);
    rg.load_grad(rel_x + r * ld, ld, lane);
    if (cfg.opt_kind == OEA_OPT_ADAGRAD) ra.load(rel_acc + r * ld, ld, lane);
    flag_t dummy;
    apply_one_row(rel + r * ld, rel_acc + r * ld, rel_x + r * ld, &dummy, ld, lane, cfg.rel_l2_norm, cfg, rv, rg, ra);
}

template <int G, int IT>
__global__ __launch_bounds__(256) void part_apply_kernel(float *__restrict__ ent, float *__restrict__ acc_own, int64_t n_ent,
                                                         float *__restrict__ rel, float *__restrict__ rel_acc, int64_t n_rel,
                                                         int ld, int world, int rank, int64_t rpr, grad_t *__restrict__ own /* [rpr*(ld+1)] */,
                                                         grad_t *__restrict__ rel_x, float *__restrict__ upd /* [rpr, ld] */,
                                                         oea_step_cfg cfg, StepWs ws, int n_partials, double *__restrict__ loss_accum) {
    const int lane = threadIdx.x % G;
    const int64_t grp = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int64_t ngrp = (int64_t)gridDim.x * blockDim.x / G;
    for (int64_t w = grp; w < rpr + n_rel; w += ngrp) {
        Row<G, IT> rv, rg, ra;
        if (w >= rpr) {
            apply_exchanged_relation_row<G, IT>(w - rpr, rel, rel_acc, n_rel, ld, lane, rel_x, cfg, rv, rg, ra);
            continue;
        }
        const int64_t j = w, id = j * world + rank;
        if (id >= n_ent) {                                         // padding slot of the last stripe
#pragma unroll
            for (int it = 0; it < IT; ++it) { const int c = it * G + lane; if (c < ld) upd[j * ld + c] = 0.f; }
            continue;
        }
        float *v = ent + id * ld;
        load_row<G, IT>(v, ld, lane, rv);
        if (own[rpr * ld + j] != 0) {
            load_grad_row<G, IT>(own + j * ld, ld, lane, rg);
            if (cfg.opt_kind == OEA_OPT_ADAGRAD) load_row<G, IT>(acc_own + j * ld, ld, lane, ra);
            flag_t dummy;
            apply_one_row(v, acc_own + j * ld, own + j * ld, &dummy, ld, lane, cfg.ent_l2_norm, cfg, rv, rg, ra);
            load_row<G, IT>(v, ld, lane, rv);                      // the updated row (same lanes wrote it)
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) { const int c = it * G + lane; if (c < ld) upd[j * ld + c] = rv.v[it]; }
    }
    if (blockIdx.x == 0 && threadIdx.x < 64) add_loss_partials_wave(ws, n_partials, loss_accum);
}

__global__ void part_unpack_kernel(float *__restrict__ ent, int64_t n_ent, int ld, int world, int rank, int64_t rpr,
                                   const float *__restrict__ all /* [G][rpr][ld] */) {
    const int cpr = ld / 4;
    const int64_t total = n_ent * cpr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t id = i / cpr;
        const int c = (int)(i - id * cpr);
        const int o = (int)(id % world);
        if (o == rank) continue;
        oea::st4(ent + id * ld + 4 * c, oea::ld4(all + ((int64_t)o * rpr + id / world) * ld + 4 * c));
    }
}

// ---- boundary-row ("halo") exchange of the partitioned step (round 5) --------------------------------------------------------------
// The dense protocol above moves every owned row every step: (G-1)/G * E * (2 ld + 1) * 4 B per rank (161 MB at the 100K shape)
// for a step that reads ~27,000 rows per rank.  BASELINE.json's north star asks for "all-gather of BOUNDARY embeddings": the rows
// a rank's share of the batch refers to.  Which rows those are is known before the step runs -- the epoch's positives and its
// negatives (drawn ahead for the whole epoch, the same Philox streams on every rank) name them -- so EVERY rank computes, for
// every step s and every rank r, the sorted list of entity rows r's share refers to, bucketed by owner (halo_mark / halo_compact;
// one copy of the [steps][G][G] counts to the host per call).  No index ever travels, the sizes of all exchanges of the call are
// known on the host, and a step is:
//   GRAD on the share -> PUSH: all-to-all of the gradient rows (+ flag) of list(s, me, o) to their owners o, added into the owner's
//   scratch (exact sums in the fixed-point build) -> relation rows all-reduced as before -> optimiser on the owned touched rows ->
//   PULL: all-to-all of the CURRENT values of list(s + 1, r, me) to the readers r of the next step.
// Rows a rank does not refer to stay stale in its local copy until the call's last step: one dense all-gather of the owned rows
// ends the range, so everything outside (evaluation, neighbour refresh, the other trainers) sees the single-GPU table.
// ~19 MB per rank and step at the 100K shape with 8 ranks (2,500 positives x (2 + 10) rows, 7/8 remote, ld + 1 floats out and ld
// back) instead of 161 MB.  TransE / TransH scores (TransD's stacked transfer rows are not in the lists: dense protocol).
struct HaloGeom {
    int world, rank;
    int64_t rpr, rpr32;            // owned rows per rank; the same rounded up to 32 (bitmap words per owner = rpr32 / 32)
    int64_t cap;                   // list entries per (step, rank)
    int nwords;                    // bitmap words per (step, rank) = world * rpr32 / 32
};

__device__ __forceinline__ void halo_mark_id(uint32_t *__restrict__ bm, const HaloGeom &g, int id) {
    const int64_t bit = (int64_t)(id % g.world) * g.rpr32 + id / g.world;
    atomicOr(bm + (bit >> 5), 1u << (bit & 31));
}

// one thread per (batch row, entry): entry 0 = the positive, 1..k its negatives; marks head and tail in the bitmap of the
// (step, rank) whose share holds the row
__global__ void halo_mark_kernel(const int32_t *__restrict__ pos_all, const int32_t *__restrict__ neg_all, int k,
                                 const int64_t *__restrict__ offsets, int s0, int s1, HaloGeom g, uint32_t *__restrict__ bitmaps) {
    const int64_t row_lo = offsets[s0], rows = offsets[s1] - row_lo;
    const int64_t total = rows * (k + 1);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = row_lo + i / (k + 1);
        const int e = (int)(i % (k + 1));
        int a = s0, b = s1;                                  // step of the row: offsets[s] <= row < offsets[s + 1]
        while (b - a > 1) { const int m = (a + b) >> 1; if (offsets[m] <= row) a = m; else b = m; }
        const int64_t b0 = offsets[a], nb = offsets[a + 1] - b0, p = row - b0;
        int r = (int)((p * g.world) / nb);
        while (r + 1 < g.world && nb * (r + 1) / g.world <= p) ++r;
        while (r > 0 && nb * r / g.world > p) --r;
        const int32_t *tr = e == 0 ? pos_all + 3 * row : neg_all + 3 * (row * k + (e - 1));
        uint32_t *bm = bitmaps + ((int64_t)(a - s0) * g.world + r) * g.nwords;
        halo_mark_id(bm, g, tr[0]);
        halo_mark_id(bm, g, tr[2]);
    }
}

// one workgroup per (step, rank): the set bits of owner o's words, ascending, as local row indices j (id = j * world + o);
// counts[(step, rank)][o]; the lists of the owners follow each other (prefix of the counts)
__global__ __launch_bounds__(256) void halo_compact_kernel(const uint32_t *__restrict__ bitmaps, HaloGeom g, int32_t *__restrict__ lists,
                                                           int32_t *__restrict__ counts, int32_t *__restrict__ err) {
    __shared__ int s_wave[4];
    __shared__ int s_base;
    const int sr = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t *bm = bitmaps + (int64_t)sr * g.nwords;
    int32_t *out = lists + (int64_t)sr * g.cap;
    const int wpo = (int)(g.rpr32 >> 5);                     // words per owner
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int o = 0; o < g.world; ++o) {
        const int start = s_base;
        for (int w0 = 0; w0 < wpo; w0 += 256) {
            const int w = w0 + tid;
            uint32_t bits = w < wpo ? bm[o * wpo + w] : 0u;
            const int c = __popc(bits);
            int incl = c;                                    // inclusive scan inside the wave
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) { const int v = __shfl_up(incl, off, 64); if (lane >= off) incl += v; }
            if (lane == 63) s_wave[wave] = incl;
            __syncthreads();
            int before = 0;
            for (int u = 0; u < wave; ++u) before += s_wave[u];
            const int chunk_total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
            int at = s_base + before + incl - c;
            while (bits) {
                const int b = __ffs(bits) - 1;
                bits &= bits - 1;
                if (at < g.cap) out[at] = w * 32 + b;
                ++at;
            }
            __syncthreads();
            if (tid == 0) s_base += chunk_total;
            __syncthreads();
        }
        if (tid == 0) counts[(int64_t)sr * g.world + o] = s_base - start;
    }
    if (tid == 0 && s_base > g.cap) atomicMax(err, 1);
}

// entry q of a concatenation of per-peer lists -> (peer, position inside the peer's list); pfx [world + 1] ascending
__device__ __forceinline__ int halo_peer_of(const int32_t *__restrict__ pfx, int world, int64_t q) {
    int a = 0, b = world;
    while (b - a > 1) { const int m = (a + b) >> 1; if (pfx[m] <= q) a = m; else b = m; }
    return a;
}

// PUSH, reader side: gradient row + flag of every remote row of list(s, me, .) -> send[q * (ld + 1)], scratch row and flag cleared
template <int G, int IT>
__global__ __launch_bounds__(256) void halo_push_pack_kernel(StepWs ws, int ld, HaloGeom g, const int32_t *__restrict__ list /* (s, me) */,
                                                             const int32_t *__restrict__ pfx /* [world + 1] over owners */,
                                                             grad_t *__restrict__ send) {
    const int lane = threadIdx.x % G;
    const int64_t grp = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G, ngrp = (int64_t)gridDim.x * blockDim.x / G;
    const int64_t total = pfx[g.world];
    for (int64_t q = grp; q < total; q += ngrp) {
        const int o = halo_peer_of(pfx, g.world, q);
        if (o == g.rank) continue;                                   // own rows stay in the scratch
        const int64_t id = (int64_t)list[q] * g.world + o;
        const flag_t f = ws.ent_touched[id];
        grad_t *dst = send + q * (ld + 1);
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int c = it * G + lane;
            if (c < ld) {
                dst[c] = f != 0 ? ws.ent_grad[id * ld + c] : (grad_t)0;
                if (f != 0) ws.ent_grad[id * ld + c] = 0;
            }
        }
        if (lane == 0) { dst[ld] = f; if (f != 0) ws.ent_touched[id] = 0; }
    }
}

// PUSH, owner side: the rows received from reader r (= list(s, r, me), known here) added into the own scratch
template <int G, int IT>
__global__ __launch_bounds__(256) void halo_push_unpack_kernel(StepWs ws, int ld, HaloGeom g, const int32_t *__restrict__ lists_s /* (s, 0) */,
                                                               const int32_t *__restrict__ own_off /* [world]: where list(s, r, me) starts in (s, r) */,
                                                               const int32_t *__restrict__ rpfx /* [world + 1] over readers */,
                                                               const grad_t *__restrict__ recv) {
    const int lane = threadIdx.x % G;
    const int64_t grp = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G, ngrp = (int64_t)gridDim.x * blockDim.x / G;
    const int64_t total = rpfx[g.world];
    for (int64_t q = grp; q < total; q += ngrp) {
        const int r = halo_peer_of(rpfx, g.world, q);
        const int64_t j = lists_s[(int64_t)r * g.cap + own_off[r] + (q - rpfx[r])];
        const int64_t id = j * g.world + g.rank;
        const grad_t *src = recv + q * (ld + 1);
        if (src[ld] == 0) continue;                                  // the reader's share left the row alone
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int c = it * G + lane;
            if (c < ld) { const grad_t v = src[c]; if (v != 0) oea::grad_add_raw(ws.ent_grad + id * ld + c, v); }
        }
        if (lane == 0) ws.ent_touched[id] = 1;
    }
}

// optimiser on the OWNED touched rows (gradient sums in the own scratch) + the relation rows from rel_x; part_apply_kernel's
// arithmetic and group widths, nothing written for the other ranks
template <int G, int IT>
__global__ __launch_bounds__(256) void halo_apply_kernel(float *__restrict__ ent, float *__restrict__ acc_own, int64_t n_ent,
                                                         float *__restrict__ rel, float *__restrict__ rel_acc, int64_t n_rel,
                                                         int ld, int world, int rank, int64_t rpr, grad_t *__restrict__ rel_x,
                                                         oea_step_cfg cfg, StepWs ws, int n_partials, double *__restrict__ loss_accum) {
    const int lane = threadIdx.x % G;
    const int64_t grp = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int64_t ngrp = (int64_t)gridDim.x * blockDim.x / G;
    for (int64_t w = grp; w < rpr + n_rel; w += ngrp) {
        Row<G, IT> rv, rg, ra;
        if (w >= rpr) {
            apply_exchanged_relation_row<G, IT>(w - rpr, rel, rel_acc, n_rel, ld, lane, rel_x, cfg, rv, rg, ra);
            continue;
        }
        const int64_t j = w, id = j * world + rank;
        if (id >= n_ent || ws.ent_touched[id] == 0) continue;
        float *v = ent + id * ld;
        load_row<G, IT>(v, ld, lane, rv);
        load_grad_row<G, IT>(ws.ent_grad + id * ld, ld, lane, rg);
        if (cfg.opt_kind == OEA_OPT_ADAGRAD) load_row<G, IT>(acc_own + j * ld, ld, lane, ra);
        apply_one_row(v, acc_own + j * ld, ws.ent_grad + id * ld, ws.ent_touched + id, ld, lane, cfg.ent_l2_norm, cfg, rv, rg, ra);
    }
    if (blockIdx.x == 0 && threadIdx.x < 64) add_loss_partials_wave(ws, n_partials, loss_accum);
}

// relation rows of the scratch (copies folded by the GRAD phase) + flags -> rel_x, scratch cleared (part_pack_kernel's relation half)
__global__ void halo_rel_pack_kernel(StepWs ws, int64_t n_rel, int ld, grad_t *__restrict__ rel_x) {
    const int64_t total = n_rel * ld;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / ld;
        const flag_t f = ws.rel_touched[r];
        rel_x[i] = f != 0 ? ws.rel_grad[i] : (grad_t)0;
        if (f != 0) ws.rel_grad[i] = 0;
    }
}
__global__ void halo_rel_flags_kernel(StepWs ws, int64_t n_rel, int ld, grad_t *__restrict__ rel_x) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_rel) { rel_x[n_rel * ld + r] = ws.rel_touched[r]; ws.rel_touched[r] = 0; }
}

// PULL: rows of the table <-> a packed buffer.  owner side (PACK): entry q of the readers' lists list(s, r, me) -> buf[q * ld];
// reader side (!PACK): buf[q * ld] -> row list(s, me, o) of owner o.  16-byte pieces.
template <bool PACK>
__global__ void halo_pull_kernel(float *__restrict__ ent, int ld, HaloGeom g, const int32_t *__restrict__ lists_s /* PACK: (s, 0); else (s, me) */,
                                 const int32_t *__restrict__ own_off, const int32_t *__restrict__ pfx, float *__restrict__ buf) {
    const int cpr = ld / 4;
    const int64_t total = (int64_t)pfx[g.world] * cpr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t q = i / cpr;
        const int c = (int)(i - q * cpr);
        const int peer = halo_peer_of(pfx, g.world, q);
        if (peer == g.rank) continue;
        if (PACK) {
            const int64_t j = lists_s[(int64_t)peer * g.cap + own_off[peer] + (q - pfx[peer])];
            oea::st4(buf + q * ld + 4 * c, oea::ld4(ent + (j * g.world + g.rank) * ld + 4 * c));
        } else {
            const int64_t j = lists_s[q];
            oea::st4(ent + (j * g.world + peer) * ld + 4 * c, oea::ld4(buf + q * ld + 4 * c));
        }
    }
}

// the owned rows -> upd [rpr, ld] (source of the dense all-gather that ends a halo range)
__global__ void halo_owned_rows_kernel(const float *__restrict__ ent, int64_t n_ent, int ld, int world, int rank, int64_t rpr,
                                       float *__restrict__ upd) {
    const int cpr = ld / 4;
    const int64_t total = rpr * cpr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = i / cpr, id = j * world + rank;
        const int c = (int)(i - j * cpr);
        oea::st4(upd + j * ld + 4 * c, id < n_ent ? oea::ld4(ent + id * ld + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f));
    }
}

}  // namespace

extern "C" {

int64_t oea_part_rows_per_rank(int64_t n_ent, int32_t world) { return world > 0 ? (n_ent + world - 1) / world : 0; }

size_t oea_part_send_floats(int64_t n_ent, int32_t ld, int32_t world) {
    return (size_t)world * (size_t)oea_part_rows_per_rank(n_ent, world) * (size_t)(ld + 1);
}

int oea_part_pack(void *workspace, int64_t n_ent, int64_t n_rel, int32_t ld, int32_t world, void *send_, void *rel_x_,
                  void *stream) {
    grad_t *send = static_cast<grad_t *>(send_), *rel_x = static_cast<grad_t *>(rel_x_);
    OEA_REQUIRE(workspace && send && rel_x && world >= 1 && ld % 4 == 0, "arguments");
    StepWs ws;
    ws_layout(n_ent, n_rel, ld, workspace, &ws);
    const int64_t rpr = oea_part_rows_per_rank(n_ent, world);
    hipStream_t st = oea::as_stream(stream);
    OEA_TRY_RC(for_row_width(ld, [&](auto g, auto it) {
        constexpr int G = decltype(g)::value;
        part_pack_kernel<G, decltype(it)::value><<<(unsigned)std::min<int64_t>(oea::ceil_div(world * rpr + n_rel, 256 / G), 16384), 256, 0, st>>>(
            ws, n_ent, n_rel, ld, world, rpr, send, rel_x);
    }));
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

int oea_part_apply(float *ent, float *acc_own, int64_t n_ent, float *rel, float *rel_acc, int64_t n_rel, int32_t ld,
                   int32_t world, int32_t rank, void *own_, void *rel_x_, float *upd, const oea_step_cfg *cfg, void *workspace,
                   int64_t n_items, double *loss_accum, void *stream) {
    grad_t *own = static_cast<grad_t *>(own_), *rel_x = static_cast<grad_t *>(rel_x_);
    OEA_REQUIRE(ent && rel && own && rel_x && upd && cfg && workspace && loss_accum, "null pointer");
    OEA_REQUIRE(world >= 1 && rank >= 0 && rank < world && ld % 4 == 0, "world / rank / ld");
    OEA_REQUIRE(cfg->opt_kind == OEA_OPT_SGD || (cfg->opt_kind == OEA_OPT_ADAGRAD && acc_own && rel_acc), "SGD or Adagrad (+ state)");
    // TransD: both stacked tables are ordinary rows; TransH: the normal-vector table goes through oea_step_apply_normals
    OEA_REQUIRE(cfg->score_kind >= OEA_SCORE_TRANSE && cfg->score_kind <= OEA_SCORE_TRANSD, "score_kind");
    StepWs ws;
    ws_layout(n_ent, n_rel, ld, workspace, &ws);
    const int64_t rpr = oea_part_rows_per_rank(n_ent, world);
    hipStream_t st = oea::as_stream(stream);
    const int n_part = loss_partials(ld, n_items);       // of the GRAD kernel that just ran on n_items work items
    OEA_TRY_RC(for_apply_width(n_ent, n_rel, ld, [&](auto g, auto it) {
        constexpr int G = decltype(g)::value;
        // the second event pair of a sampled step (the GRAD call took the first): bench.py's apply timing under partitioning
        oea::launch_timed(part_apply_kernel<G, decltype(it)::value>,
                          (unsigned)std::min<int64_t>(std::max<int64_t>(oea::ceil_div(rpr + n_rel, 256 / G), 1), 16384), 256, st, ent, acc_own,
                          n_ent, rel, rel_acc, n_rel, ld, world, rank, rpr, own, rel_x, upd, *cfg, ws, n_part, loss_accum);
    }));
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

int oea_part_unpack(float *ent, int64_t n_ent, int32_t ld, int32_t world, int32_t rank, const float *all, void *stream) {
    OEA_REQUIRE(ent && all && world >= 1 && rank >= 0 && rank < world && ld % 4 == 0, "arguments");
    if (world == 1) return OEA_OK;
    const int64_t rpr = oea_part_rows_per_rank(n_ent, world);
    part_unpack_kernel<<<(unsigned)std::min<int64_t>(oea::ceil_div(n_ent * (ld / 4), 256), 16384), 256, 0, oea::as_stream(stream)>>>(
        ent, n_ent, ld, world, rank, rpr, all);
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

}  // extern "C"

// ---- ONE walk over the batches of an epoch's step range: the plain, the partitioned and the boundary-row epoch ---------------------
static_assert(sizeof(oea_epoch) == 184, "oea_epoch: openea_amd/_lib.py:Epoch and tests/test_host_cpu.py hold the same layout");

struct EpochStep {                    // a non-empty batch of the range, cut to this rank's share (which may be empty: n == 0)
    int32_t s;                        // its step inside the epoch
    int64_t lo, n, r_lo, split;       // rows [lo, lo + n) of pos_all = the batch's rows from r_lo on, the first `split` of them from KG1
    const int32_t *pos;
    int32_t *negs;                    // the share's n * k negatives (drawn when the step body runs); NULL when k == 0
};

struct EpochWalk {
    const oea_epoch *e;
    int32_t step_begin, step_end, rank, world;
    bool presampled, ahead, sample_all;
    int64_t max_batch;                // the epoch's largest batch
    oea_step_cfg cfg;                 // the running step's: Adam's opt_t counts the steps actually run (e->cfg->opt_t = count of the first)
    void *stream;
};

// validates what the three forms share, decides where the negatives come from and draws the whole epoch's when the range starts it
static int epoch_walk_begin(const oea_epoch *e, int32_t step_begin, int32_t step_end, int32_t rank, int32_t world, void *stream,
                            EpochWalk *w) {
    OEA_REQUIRE(e && e->pos_all && e->offsets_host && e->splits_host && e->cfg, "null pointer");
    OEA_REQUIRE(e->steps >= 0 && e->k >= 0, "steps, k >= 0");
    OEA_REQUIRE(0 <= step_begin && step_begin <= step_end && step_end <= e->steps, "0 <= step_begin <= step_end <= steps");
    OEA_REQUIRE((e->offsets_dev == nullptr) == (e->splits_dev == nullptr), "offsets_dev and splits_dev go together");
    OEA_REQUIRE(world >= 1 && rank >= 0 && rank < world, "0 <= rank < world");
    const int32_t k = e->k, steps = e->steps;
    // side0 == NULL with the device layout given: neg_buf already holds the epoch's negatives (the caller drew them
    // with oea_sample_negatives_epoch, e.g. on another stream while the previous epoch was running)
    const bool presampled = k > 0 && e->side0 == nullptr && e->side1 == nullptr && e->offsets_dev != nullptr;
    OEA_REQUIRE(k == 0 || (e->neg_buf && (presampled || (e->err_flag && e->side0 && e->side1))),
                "sampling needs neg_buf, err_flag and both sides");
    const bool ahead = k > 0 && e->offsets_dev != nullptr && steps > 0;      // neg_buf covers the whole epoch
    // the sampler does not read the tables: a range that starts the epoch draws ALL its negatives in one launch
    // (later ranges of the same epoch find them in neg_buf: pass side0 = side1 = NULL, or let them be drawn again
    // step by step -- the Philox streams are the same either way).  A rank of a sharded job draws the WHOLE epoch as
    // well (same streams on every rank: the union of the ranks' slices is the single-process draw) and uses its rows.
    const bool sample_all = ahead && !presampled && step_begin == 0;
    if (sample_all)
        OEA_TRY_RC(oea_sample_negatives_epoch(e->pos_all, e->offsets_host[steps], e->offsets_dev, e->splits_dev, steps, k, e->side0, e->side1,
                                              e->seed, e->step_base, 10, e->neg_buf, e->err_flag, stream));
    int64_t max_batch = 0;
    for (int32_t s = 0; s < steps; ++s) max_batch = std::max(max_batch, e->offsets_host[s + 1] - e->offsets_host[s]);
    *w = EpochWalk{e, step_begin, step_end, rank, world, presampled, ahead, sample_all, max_batch, *e->cfg, stream};
    return OEA_OK;
}

// step(EpochStep) -> OEA_* for every non-empty batch of the range, with w.cfg the step's configuration
template <class F>
static int epoch_walk(EpochWalk &w, F &&step) {
    const oea_epoch &e = *w.e;
    for (int32_t s = w.step_begin; s < w.step_end; ++s) {
        const int64_t b0 = e.offsets_host[s], nb = e.offsets_host[s + 1] - b0;
        if (nb <= 0) continue;
        // this rank's contiguous share of the batch rows (models/dist.py:shard_batch; the whole batch when world == 1)
        const int64_t r_lo = nb * w.rank / w.world, r_hi = nb * (w.rank + 1) / w.world;
        const int64_t lo = b0 + r_lo, n = r_hi - r_lo;
        const int64_t split = std::min(std::max<int64_t>(e.splits_host[s] - r_lo, 0), n);
        int32_t *negs = e.k == 0 ? nullptr : w.ahead ? e.neg_buf + 3 * lo * (int64_t)e.k : e.neg_buf;
        const EpochStep t{s, lo, n, r_lo, split, e.pos_all + 3 * lo, negs};
        if (n > 0 && e.k > 0 && !w.presampled && !w.sample_all)
            OEA_TRY_RC(oea_sample_negatives_pair(t.pos, n, split, e.k, e.side0, e.side1, e.seed, e.step_base + (uint32_t)s, (uint32_t)r_lo, 10,
                                                 negs, e.err_flag, w.stream));
        OEA_TRY_RC(step(t));
        ++w.cfg.opt_t;
    }
    return OEA_OK;
}

// ---- the halo form of the one-call partitioned epoch ---------------------------------------------------------------------------------
static HaloGeom halo_geom(int64_t n_ent, int32_t world, int32_t rank, int64_t max_batch, int32_t k) {
    HaloGeom g;
    g.world = world; g.rank = rank;
    g.rpr = oea_part_rows_per_rank(n_ent, world);
    g.rpr32 = (g.rpr + 31) / 32 * 32;
    g.nwords = (int)((int64_t)world * g.rpr32 / 32);
    const int64_t share = oea::ceil_div(max_batch, world) + 1;
    g.cap = std::min<int64_t>(2 * share * (1 + (int64_t)k), (int64_t)world * g.rpr);
    g.cap = (g.cap + 3) / 4 * 4;
    return g;
}
struct HaloWs { uint32_t *bitmaps; int32_t *lists, *counts, *tables, *err; };
// tables: per step [4][world + 1] int32: 0 = prefix over owners of count(s, me, .), 1 = prefix over readers of count(s, ., me) (me
// excluded), 2 = where list(s, r, me) starts inside (s, r) (index r), 3 = spare
static size_t halo_ws_layout(const HaloGeom &g, int32_t steps, void *base, HaloWs *ws) {
    size_t off = 0;
    char *b = static_cast<char *>(base);
    auto take = [&](size_t bytes) { size_t o = off; off += align256(bytes); return b ? b + o : nullptr; };
    uint32_t *bm = (uint32_t *)take(4 * (size_t)steps * g.world * g.nwords);
    int32_t *li = (int32_t *)take(4 * (size_t)steps * g.world * g.cap);
    int32_t *co = (int32_t *)take(4 * (size_t)steps * g.world * g.world);
    int32_t *ta = (int32_t *)take(4 * (size_t)steps * 4 * (g.world + 1));
    int32_t *er = (int32_t *)take(256);
    if (ws) { ws->bitmaps = bm; ws->lists = li; ws->counts = co; ws->tables = ta; ws->err = er; }
    return off;
}

// the row lists of steps [step_begin, step_end): who refers to which rows in which step -> hw.lists / hw.counts, hw.err = overflow
static int halo_build_lists(const int32_t *pos_all, const int32_t *neg_all, int32_t k, const int64_t *offsets_host,
                            const int64_t *offsets_dev, int32_t step_begin, int32_t step_end, const HaloGeom &g, const HaloWs &hw,
                            hipStream_t st) {
    const int32_t nS = step_end - step_begin;
    OEA_CHECK_HIP(hipMemsetAsync(hw.bitmaps, 0, 4 * (size_t)nS * g.world * g.nwords, st));
    OEA_CHECK_HIP(hipMemsetAsync(hw.err, 0, 4, st));
    const int64_t rows = offsets_host[step_end] - offsets_host[step_begin];
    if (rows > 0)
        halo_mark_kernel<<<(unsigned)std::min<int64_t>(oea::ceil_div(rows * (k + 1), 256), 16384), 256, 0, st>>>(
            pos_all, neg_all, k, offsets_dev, step_begin, step_end, g, hw.bitmaps);
    halo_compact_kernel<<<(unsigned)(nS * g.world), 256, 0, st>>>(hw.bitmaps, g, hw.lists, hw.counts, hw.err);
    return OEA_OK;
}

extern "C" {

int oea_triple_epoch_range(const oea_epoch *e, int32_t step_begin, int32_t step_end, int32_t rank, int32_t world, void *plan,
                           size_t plan_bytes, int32_t plan_built, void *stream) {
    EpochWalk w;
    OEA_TRY_RC(epoch_walk_begin(e, step_begin, step_end, rank, world, stream, &w));
    // the gathered-sum plan (step_plan.h): needs the whole epoch's negatives to exist before its first step
    oea::StepPlanView pv;
    const bool use_plan = plan && world == 1 && w.ahead && (w.presampled || w.sample_all) &&
                          oea_step_plan_supported(e->cfg, e->n_ent, e->n_rel, e->ld, e->k);
    if (use_plan) {
        const int64_t n_total = e->offsets_host[e->steps];
        const size_t need = oea::step_plan_layout(n_total, e->steps, w.max_batch, e->n_ent, e->ld, plan, &pv);
        OEA_REQUIRE(plan_bytes >= need, "plan workspace smaller than oea_step_plan_bytes");
        if (!plan_built)
            OEA_TRY_RC(oea_step_plan_build(e->pos_all, e->neg_buf, e->k, e->offsets_dev, n_total, e->steps, w.max_batch, e->n_ent, e->ld, plan,
                                           plan_bytes, stream));
    }
    return epoch_walk(w, [&](const EpochStep &t) -> int {
        if (t.n == 0) return OEA_OK;
        return oea::step_phase_planned(e->ent, e->ent_acc, e->n_ent, e->rel, e->rel_acc, e->n_rel, e->dim, e->ld, t.pos, t.n, t.negs,
                                       t.n * (int64_t)e->k, &w.cfg, e->workspace, e->loss_accum, OEA_PHASE_BOTH, stream,
                                       use_plan ? &pv : nullptr, t.s, t.lo);
    });
}

// The steps [step_begin, step_end) of a data-parallel epoch under the entity-id partition, enqueued by ONE call: per step
// GRAD on this rank's share of the batch -> pack -> reduce-scatter (RCCL) + all-reduce of the relation rows -> optimiser on
// the owned rows -> all-gather -> unpack; everything on `stream`, no host work between the steps (driven from Python the
// exchange costs six library calls and three torch.distributed calls per step).  The communicator is the C ABI's own
// (oea_comm_*: RCCL through dlopen), so a non-Python host runs the same job.  Buffers as in the step-by-step protocol
// (include/openea_hip.h): send [world * rpr * (ld + 1)], own [rpr * (ld + 1)], rel_x [n_rel * (ld + 1)], upd [rpr, ld],
// all [world, rpr, ld]; e->ent_acc = the optimiser state of the owned rows.  TransH: the normal vectors' scratch is all-reduced
// and applied on every rank.  Same Philox streams as the single-GPU epoch; result = the step-by-step partitioned job.
int oea_triple_epoch_range_comm(oea_comm_t comm, const oea_epoch *e, int32_t step_begin, int32_t step_end, void *send, void *own,
                                void *rel_x, float *upd, float *all, void *stream) {
    OEA_REQUIRE(comm && e && e->pos_all && e->offsets_host && e->splits_host && e->cfg && send && own && rel_x && upd && all, "null pointer");
    OEA_REQUIRE(e->steps >= 0 && e->k >= 0 && 0 <= step_begin && step_begin <= step_end && step_end <= e->steps, "step range");
    OEA_REQUIRE(e->cfg->opt_kind == OEA_OPT_SGD || e->cfg->opt_kind == OEA_OPT_ADAGRAD, "the partition runs SGD / Adagrad");
    const int32_t world = oea_comm_size(comm), rank = oea_comm_rank(comm);
    EpochWalk w;
    OEA_TRY_RC(epoch_walk_begin(e, step_begin, step_end, rank, world, stream, &w));
    const int64_t n_ent = e->n_ent, n_rel = e->n_rel;
    const int32_t ld = e->ld, k = e->k;
    const int64_t rpr = oea_part_rows_per_rank(n_ent, world);
    const int64_t chunk = rpr * (ld + 1);
    const bool transh = e->cfg->score_kind == OEA_SCORE_TRANSH;
    StepWs ws;                                 // (TransH: where the normals' scratch and flags sit)
    ws_layout(n_ent, n_rel, ld, e->workspace, &ws);
    // the gradients travel in the scratch's own type: fp32, or int64 fixed point in the deterministic build (exact sums:
    // the G-rank job then equals the single-GPU job bit for bit)
    const int32_t gdt = oea::kDetScratch ? OEA_COMM_I64 : OEA_COMM_F32;
    hipStream_t st = oea::as_stream(stream);
    return epoch_walk(w, [&](const EpochStep &t) -> int {
        // every rank takes part in every exchange, also with an empty share of the batch (n == 0: nothing scored)
        OEA_TRY_RC(oea::comm_phase_mark(comm, st));
        OEA_TRY_RC(oea_triple_step_phase(e->ent, nullptr, n_ent, e->rel, e->rel_acc, n_rel, e->dim, ld, t.pos, t.n, t.negs, t.n * (int64_t)k,
                                         &w.cfg, e->workspace, e->loss_accum, OEA_PHASE_GRAD, stream));
        OEA_TRY_RC(oea::comm_phase_mark(comm, st));
        OEA_TRY_RC(oea_part_pack(e->workspace, n_ent, n_rel, ld, world, send, rel_x, stream));
        OEA_TRY_RC(oea::comm_phase_mark(comm, st));
        OEA_TRY_RC(oea_comm_reduce_scatter(comm, send, own, chunk, gdt, stream));
        OEA_TRY_RC(oea_comm_allreduce(comm, rel_x, n_rel * (int64_t)(ld + 1), gdt, stream));
        if (transh) {
            OEA_TRY_RC(oea_comm_allreduce(comm, ws.nrm_grad, n_rel * (int64_t)ld, gdt, stream));
            OEA_TRY_RC(oea_comm_allreduce(comm, ws.nrm_touched, n_rel, gdt, stream));
        }
        OEA_TRY_RC(oea::comm_phase_mark(comm, st));
        OEA_TRY_RC(oea_part_apply(e->ent, e->ent_acc, n_ent, e->rel, e->rel_acc, n_rel, ld, world, rank, own, rel_x, upd, &w.cfg, e->workspace,
                                  step_items(w.cfg, t.n, t.n * (int64_t)k), e->loss_accum, stream));
        if (transh) OEA_TRY_RC(oea_step_apply_normals(n_ent, n_rel, ld, &w.cfg, e->workspace, stream));
        OEA_TRY_RC(oea::comm_phase_mark(comm, st));
        OEA_TRY_RC(oea_allgather_rows(comm, upd, all, rpr, ld, stream));
        OEA_TRY_RC(oea::comm_phase_mark(comm, st));
        OEA_TRY_RC(oea_part_unpack(e->ent, n_ent, ld, world, rank, all, stream));
        return oea::comm_phase_mark(comm, st);
    });
}

size_t oea_halo_workspace_bytes(int64_t n_ent, int32_t world, int32_t steps, int64_t max_batch, int32_t k) {
    if (world < 1 || steps < 0) return 0;
    return halo_ws_layout(halo_geom(n_ent, world, 0, max_batch, k), steps, nullptr, nullptr);
}

// bytes of EACH of the two exchange buffers: the larger of what a rank can send (its lists: <= cap rows) and receive (the other
// ranks' lists of its rows: <= (world - 1) * min(cap, rpr) rows), ld + 1 scratch elements per row
size_t oea_halo_buffer_bytes(int64_t n_ent, int32_t world, int64_t max_batch, int32_t k, int32_t ld) {
    if (world < 1) return 0;
    const HaloGeom g = halo_geom(n_ent, world, 0, max_batch, k);
    const int64_t rows = std::max<int64_t>(g.cap, (int64_t)(world - 1) * std::min<int64_t>(g.cap, g.rpr));
    return align256((size_t)rows * (ld + 1) * sizeof(grad_t));
}

// the plan alone: counts_host [step_end - step_begin][world][world] = distinct rows rank r's share of step s refers to that rank o owns
// (what sizes every message of oea_triple_epoch_range_halo), lists_host (may be NULL) [steps][world][cap] the row lists themselves
// (local indices j, id = j * world + owner, owner-major, ascending); *cap_out = entries per (step, rank).  Parity: tests hold both to
// a numpy restatement (oracle/np_oracle.py:halo_plan).
int oea_halo_plan(const int32_t *pos_all, const int32_t *neg_all, int32_t k, const int64_t *offsets_host, const int64_t *offsets_dev,
                  int32_t steps, int32_t step_begin, int32_t step_end, int64_t n_ent, int32_t world, void *halo_ws, size_t halo_ws_bytes,
                  int32_t *counts_host, int32_t *lists_host, int64_t *cap_out, void *stream) {
    OEA_REQUIRE(pos_all && offsets_host && offsets_dev && halo_ws && counts_host, "null pointer");
    OEA_REQUIRE(steps >= 0 && k >= 0 && (k == 0 || neg_all) && 0 <= step_begin && step_begin <= step_end && step_end <= steps && world >= 1, "arguments");
    hipStream_t st = oea::as_stream(stream);
    const int32_t nS = step_end - step_begin;
    int64_t max_batch = 0;
    for (int32_t s = 0; s < steps; ++s) max_batch = std::max(max_batch, offsets_host[s + 1] - offsets_host[s]);
    const HaloGeom g = halo_geom(n_ent, world, 0, max_batch, k);
    if (cap_out) *cap_out = g.cap;
    if (nS == 0) return OEA_OK;
    HaloWs hw;
    OEA_REQUIRE(halo_ws_bytes >= halo_ws_layout(g, nS, halo_ws, &hw), "halo workspace smaller than oea_halo_workspace_bytes");
    OEA_TRY_RC(halo_build_lists(pos_all, neg_all, k, offsets_host, offsets_dev, step_begin, step_end, g, hw, st));
    int32_t err = 0;
    OEA_CHECK_HIP(hipMemcpyAsync(counts_host, hw.counts, 4 * (size_t)nS * world * world, hipMemcpyDeviceToHost, st));
    if (lists_host) OEA_CHECK_HIP(hipMemcpyAsync(lists_host, hw.lists, 4 * (size_t)nS * world * g.cap, hipMemcpyDeviceToHost, st));
    OEA_CHECK_HIP(hipMemcpyAsync(&err, hw.err, 4, hipMemcpyDeviceToHost, st));
    OEA_CHECK_HIP(hipStreamSynchronize(st));
    OEA_REQUIRE(err == 0, "halo lists overflowed their capacity");
    return OEA_OK;
}

int oea_triple_epoch_range_halo(oea_comm_t comm, const oea_epoch *e, int32_t step_begin, int32_t step_end, void *halo_ws,
                                size_t halo_ws_bytes, void *buf_a, void *buf_b, size_t buf_bytes, void *rel_x, float *upd, float *all,
                                int64_t *stats_host, void *stream) {
    OEA_REQUIRE(comm && e && e->ent && e->rel && e->pos_all && e->offsets_host && e->splits_host && e->cfg && e->workspace && e->loss_accum &&
                halo_ws && buf_a && buf_b && rel_x && upd && all, "null pointer");
    OEA_REQUIRE(e->steps >= 0 && e->k >= 0 && 0 <= step_begin && step_begin <= step_end && step_end <= e->steps, "step range");
    OEA_REQUIRE(e->offsets_dev && e->splits_dev, "the halo exchange plans from the epoch's batches on the device: offsets_dev / splits_dev");
    OEA_REQUIRE(e->cfg->opt_kind == OEA_OPT_SGD || e->cfg->opt_kind == OEA_OPT_ADAGRAD, "the partition runs SGD / Adagrad");
    OEA_REQUIRE(e->cfg->score_kind == OEA_SCORE_TRANSE || e->cfg->score_kind == OEA_SCORE_TRANSH, "halo exchange: TransE / TransH scores");
    OEA_REQUIRE(e->ld % 4 == 0, "ld % 4 == 0");
    const int32_t world = oea_comm_size(comm), rank = oea_comm_rank(comm);
    EpochWalk w;
    OEA_TRY_RC(epoch_walk_begin(e, step_begin, step_end, rank, world, stream, &w));
    // (a range that does not start the epoch drew nothing above: its steps would be sampled one by one, after the lists are built)
    OEA_REQUIRE(e->k == 0 || w.presampled || step_begin == 0, "the whole epoch's negatives are drawn by the range that starts it");
    const int64_t n_ent = e->n_ent, n_rel = e->n_rel;
    const int32_t ld = e->ld, k = e->k;
    const int64_t *offsets_host = e->offsets_host;
    float *ent = e->ent;
    hipStream_t st = oea::as_stream(stream);
    const int32_t nS = step_end - step_begin;
    if (stats_host) { stats_host[0] = stats_host[1] = stats_host[2] = stats_host[3] = 0; }
    if (nS == 0) return OEA_OK;
    const HaloGeom g = halo_geom(n_ent, world, rank, w.max_batch, k);
    HaloWs hw;
    OEA_REQUIRE(halo_ws_bytes >= halo_ws_layout(g, nS, halo_ws, &hw), "halo workspace smaller than oea_halo_workspace_bytes(n_ent, world, steps, max_batch, k)");
    OEA_REQUIRE(buf_bytes >= oea_halo_buffer_bytes(n_ent, world, w.max_batch, k, ld), "exchange buffers smaller than oea_halo_buffer_bytes");
    // ---- plan: who refers to which rows in which step (every rank computes the same tables) -----------------------------------
    OEA_TRY_RC(halo_build_lists(e->pos_all, e->neg_buf, k, offsets_host, e->offsets_dev, step_begin, step_end, g, hw, st));
    std::vector<int32_t> counts((size_t)nS * world * world + 1);
    OEA_CHECK_HIP(hipMemcpyAsync(counts.data(), hw.counts, 4 * (size_t)nS * world * world, hipMemcpyDeviceToHost, st));
    OEA_CHECK_HIP(hipMemcpyAsync(counts.data() + (size_t)nS * world * world, hw.err, 4, hipMemcpyDeviceToHost, st));
    OEA_CHECK_HIP(hipStreamSynchronize(st));                          // the ONE host read of the call
    OEA_REQUIRE(counts[(size_t)nS * world * world] == 0, "halo lists overflowed their capacity (entries of a batch that are not corruptions?)");
    auto cnt = [&](int s, int r, int o) { return (int64_t)counts[((size_t)s * world + r) * world + o]; };
    std::vector<int32_t> tables((size_t)nS * 4 * (world + 1), 0);
    for (int s = 0; s < nS; ++s) {
        int32_t *t0 = tables.data() + (size_t)s * 4 * (world + 1), *t1 = t0 + (world + 1), *t2 = t1 + (world + 1);
        for (int o = 0; o < world; ++o) t0[o + 1] = t0[o] + (int32_t)cnt(s, rank, o);
        for (int r = 0; r < world; ++r) {
            t1[r + 1] = t1[r] + (r == rank ? 0 : (int32_t)cnt(s, r, rank));
            int32_t off = 0;
            for (int o = 0; o < rank; ++o) off += (int32_t)cnt(s, r, o);
            t2[r] = off;
        }
    }
    OEA_CHECK_HIP(hipMemcpyAsync(hw.tables, tables.data(), 4 * tables.size(), hipMemcpyHostToDevice, st));
    OEA_CHECK_HIP(hipStreamSynchronize(st));                          // (tables lives on this stack frame)
    const int64_t rpr = g.rpr;
    const bool transh = e->cfg->score_kind == OEA_SCORE_TRANSH;
    const int32_t gdt = oea::kDetScratch ? OEA_COMM_I64 : OEA_COMM_F32;
    StepWs ws;
    ws_layout(n_ent, n_rel, ld, e->workspace, &ws);
    grad_t *xa = static_cast<grad_t *>(buf_a), *xb = static_cast<grad_t *>(buf_b), *relx = static_cast<grad_t *>(rel_x);
    std::vector<int64_t> sc(world), sd(world), rc_(world), rd(world);
    OEA_TRY_RC(epoch_walk(w, [&](const EpochStep &t) -> int {
        const int32_t s = t.s;
        const int sl = s - step_begin;
        const int32_t *tab = hw.tables + (size_t)sl * 4 * (world + 1);
        const int32_t *t0h = tables.data() + (size_t)sl * 4 * (world + 1), *t1h = t0h + (world + 1);
        OEA_TRY_RC(oea::comm_phase_mark(comm, st));
        OEA_TRY_RC(oea_triple_step_phase(ent, nullptr, n_ent, e->rel, e->rel_acc, n_rel, e->dim, ld, t.pos, t.n, t.negs, t.n * (int64_t)k, &w.cfg,
                                         e->workspace, e->loss_accum, OEA_PHASE_GRAD, stream));
        OEA_TRY_RC(oea::comm_phase_mark(comm, st));
        // ---- PUSH -------------------------------------------------------------------------------------------------------------
        const int64_t n_send = t0h[world], n_recv = t1h[world];
        const int32_t *list_me = hw.lists + ((size_t)sl * world + rank) * g.cap, *lists_s = hw.lists + (size_t)sl * world * g.cap;
        OEA_TRY_RC(for_row_width(ld, [&](auto gw, auto it) {
            constexpr int G = decltype(gw)::value;
            if (n_send > 0)
                halo_push_pack_kernel<G, decltype(it)::value><<<(unsigned)std::min<int64_t>(oea::ceil_div(n_send, 256 / G), 16384), 256, 0, st>>>(
                    ws, ld, g, list_me, tab, xa);
        }));
        halo_rel_pack_kernel<<<(unsigned)std::min<int64_t>(oea::ceil_div(n_rel * (int64_t)ld, 256), 4096), 256, 0, st>>>(ws, n_rel, ld, relx);
        halo_rel_flags_kernel<<<(unsigned)oea::ceil_div(n_rel, 256), 256, 0, st>>>(ws, n_rel, ld, relx);
        OEA_TRY_RC(oea::comm_phase_mark(comm, st));
        for (int p = 0; p < world; ++p) {
            sc[p] = p == rank ? 0 : cnt(sl, rank, p) * (ld + 1);
            sd[p] = (int64_t)t0h[p] * (ld + 1);
            rc_[p] = p == rank ? 0 : cnt(sl, p, rank) * (ld + 1);
            rd[p] = (int64_t)t1h[p] * (ld + 1);
        }
        OEA_TRY_RC(oea_comm_alltoallv(comm, xa, sc.data(), sd.data(), xb, rc_.data(), rd.data(), gdt, stream));
        OEA_TRY_RC(oea_comm_allreduce(comm, relx, n_rel * (int64_t)(ld + 1), gdt, stream));
        if (transh) {
            OEA_TRY_RC(oea_comm_allreduce(comm, ws.nrm_grad, n_rel * (int64_t)ld, gdt, stream));
            OEA_TRY_RC(oea_comm_allreduce(comm, ws.nrm_touched, n_rel, gdt, stream));
        }
        if (stats_host) {
            int64_t out_rows = 0;
            for (int p = 0; p < world; ++p) out_rows += p == rank ? 0 : cnt(sl, rank, p);
            stats_host[0] += out_rows * (ld + 1) * (int64_t)sizeof(grad_t);
            stats_host[2] = std::max(stats_host[2], out_rows);
            stats_host[3] += 1;
        }
        OEA_TRY_RC(oea::comm_phase_mark(comm, st));
        OEA_TRY_RC(for_row_width(ld, [&](auto gw, auto it) {
            constexpr int G = decltype(gw)::value;
            if (n_recv > 0)
                halo_push_unpack_kernel<G, decltype(it)::value><<<(unsigned)std::min<int64_t>(oea::ceil_div(n_recv, 256 / G), 16384), 256, 0, st>>>(
                    ws, ld, g, lists_s, tab + 2 * (world + 1), tab + (world + 1), xb);
        }));
        // ---- optimiser on the owned rows (the single-GPU job's group width at this table size) ---------------------------------
        const int n_part = loss_partials(ld, step_items(w.cfg, t.n, t.n * (int64_t)k));
        OEA_TRY_RC(for_apply_width(n_ent, n_rel, ld, [&](auto gw, auto it) {
            constexpr int G = decltype(gw)::value;
            oea::launch_timed(halo_apply_kernel<G, decltype(it)::value>,
                              (unsigned)std::min<int64_t>(std::max<int64_t>(oea::ceil_div(rpr + n_rel, 256 / G), 1), 16384), 256, st, ent,
                              e->ent_acc, n_ent, e->rel, e->rel_acc, n_rel, ld, world, rank, rpr, relx, w.cfg, ws, n_part, e->loss_accum);
        }));
        if (transh) OEA_TRY_RC(oea_step_apply_normals(n_ent, n_rel, ld, &w.cfg, e->workspace, stream));
        OEA_TRY_RC(oea::comm_phase_mark(comm, st));
        // ---- PULL for the next step of the range: the current values of the rows its readers refer to ---------------------------
        int32_t s2 = s + 1;
        while (s2 < step_end && offsets_host[s2 + 1] - offsets_host[s2] <= 0) ++s2;
        if (s2 < step_end) {
            const int sl2 = s2 - step_begin;
            const int32_t *tab2 = hw.tables + (size_t)sl2 * 4 * (world + 1);
            const int32_t *u0 = tables.data() + (size_t)sl2 * 4 * (world + 1), *u1 = u0 + (world + 1);
            const int64_t n_out = u1[world], n_in = u0[world];
            float *fa = reinterpret_cast<float *>(xa), *fb = reinterpret_cast<float *>(xb);
            if (n_out > 0)
                halo_pull_kernel<true><<<(unsigned)std::min<int64_t>(oea::ceil_div(n_out * (ld / 4), 256), 16384), 256, 0, st>>>(
                    ent, ld, g, hw.lists + (size_t)sl2 * world * g.cap, tab2 + 2 * (world + 1), tab2 + (world + 1), fb);
            for (int p = 0; p < world; ++p) {
                sc[p] = p == rank ? 0 : cnt(sl2, p, rank) * ld;
                sd[p] = (int64_t)u1[p] * ld;
                rc_[p] = p == rank ? 0 : cnt(sl2, rank, p) * ld;
                rd[p] = (int64_t)u0[p] * ld;
            }
            OEA_TRY_RC(oea_comm_alltoallv(comm, fb, sc.data(), sd.data(), fa, rc_.data(), rd.data(), OEA_COMM_F32, stream));
            OEA_TRY_RC(oea::comm_phase_mark(comm, st));
            if (n_in > 0)
                halo_pull_kernel<false><<<(unsigned)std::min<int64_t>(oea::ceil_div(n_in * (ld / 4), 256), 16384), 256, 0, st>>>(
                    ent, ld, g, hw.lists + ((size_t)sl2 * world + rank) * g.cap, nullptr, tab2, fa);
            if (stats_host) {
                int64_t in_rows = 0;
                for (int p = 0; p < world; ++p) in_rows += p == rank ? 0 : cnt(sl2, rank, p);
                stats_host[1] += in_rows * ld * 4;
            }
        } else {
            // the range ends: one dense all-gather of the owned rows makes every copy the single-GPU table
            halo_owned_rows_kernel<<<(unsigned)std::min<int64_t>(oea::ceil_div(rpr * (ld / 4), 256), 16384), 256, 0, st>>>(ent, n_ent, ld, world, rank, rpr, upd);
            OEA_TRY_RC(oea_allgather_rows(comm, upd, all, rpr, ld, stream));
            OEA_TRY_RC(oea::comm_phase_mark(comm, st));
            OEA_TRY_RC(oea_part_unpack(ent, n_ent, ld, world, rank, all, stream));
        }
        return oea::comm_phase_mark(comm, st);
    }));
    OEA_CHECK_HIP(hipGetLastError());
    return OEA_OK;
}

}  // extern "C"
