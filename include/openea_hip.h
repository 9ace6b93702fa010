/*
 * openea_hip.h -- C ABI of libopenea_hip.so: the MI355X (gfx950) implementation of OpenEA's
 * training / evaluation hot path.
 *
 * The reference (nju-websoft/OpenEA) has NO FFI of its own: the path runs as TensorFlow-1 stock
 * ops plus numpy/scipy calls.  Each entry point below therefore names the reference call site
 * (file:line relative to /root/reference/src/openea/) whose arithmetic it replaces; the Python
 * mirror of the reference's module API (openea_amd/modules/...) is the only caller.
 * INTEGRATION.md shows the ctypes binding a reference maintainer would add.
 *
 * Conventions
 *   - plain C: pointers + sizes, no torch / C++ types.
 *   - every `*_dev` / unqualified data pointer is a HIP DEVICE pointer unless the name ends in
 *     `_host`; `stream` is a hipStream_t passed as void* (NULL = default stream).
 *   - all functions return 0 on success, a negative OEA_E* code otherwise;
 *     oea_last_error() returns a thread-local message for the last failure.
 *   - tables are fp32 row-major [rows, ld] with ld >= dim and ld % 4 == 0; columns
 *     [dim, ld) must be zero and are kept zero.  ids are int32.  Triples are int32 [n,3]
 *     (head, relation, tail) interleaved.
 *   - calls are asynchronous on `stream`; the caller synchronises.  Not re-entrant on the
 *     same buffers.
 */
#ifndef OPENEA_HIP_H
#define OPENEA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OEA_OK 0
#define OEA_EINVAL (-1)   /* bad argument */
#define OEA_EHIP (-2)     /* HIP runtime error */
#define OEA_ENOMEM (-3)
#define OEA_EUNSUPPORTED (-4)

int oea_version(void);
const char *oea_last_error(void);
/* number of visible HIP devices, <0 on error (used by the host side to fail loudly) */
int oea_device_count(void);

/* Per-kernel timing with HIP events on the launch stream (used by bench.py for the roofline
 * figure; no reference counterpart).  Between begin and end, every sampled optimiser step carries 4
 * events: [m0 fwd_bwd kernel m1] [m2 apply kernel m3] (a GRAD-phase call the first pair, the
 * APPLY-phase call the second), each pair ATTACHED to its kernel's dispatch (hipExtLaunchKernelGGL
 * start / stop events = the dispatch's own begin / end timestamps, the figure rocprofv3's kernel
 * trace reports) rather than recorded as separate barrier packets around it.  oea_profile_end(4, ms, &n) returns ms[0] = total fwd_bwd
 * time, ms[1] = time between the two kernels (the exchange under data parallelism), ms[2] = total
 * apply time (milliseconds) over n steps.
 * stride: only every stride-th step records its marks (an event record costs a few microseconds of
 * enqueue time, comparable to the kernels themselves at the 15K shape). */
int oea_profile_begin(int32_t stride);
int oea_profile_end(int32_t group, double *out_ms_host, int32_t *n_calls_host);

/* ---------------------------------------------------------------------------------------
 * Embedding store -- replaces the tf.Variable tables of BasicModel._define_variables
 * (models/basic_model.py:73-78) and their .eval() round trips (basic_model.py:106-121,
 * 184-204).  Payload layout of load/save_host == the C-contiguous fp32 [rows, dim] payload
 * of ent_embeds.npy (modules/load/read.py:325-349).
 * ------------------------------------------------------------------------------------- */
typedef struct oea_store *oea_store_t;
int oea_store_create(int64_t rows, int32_t dim, oea_store_t *out);
int oea_store_destroy(oea_store_t s);
int64_t oea_store_rows(oea_store_t s);
int32_t oea_store_dim(oea_store_t s);
int32_t oea_store_ld(oea_store_t s);
float *oea_store_rows_ptr(oea_store_t s);                       /* device pointer [rows, ld] */
int oea_store_load_host(oea_store_t s, const float *src_host, void *stream);  /* [rows, dim] */
int oea_store_save_host(oea_store_t s, float *dst_host, void *stream);        /* [rows, dim] */

/* out[i, 0:dim] = table[ids[i]] (optionally row-L2-normalised: tf.nn.l2_normalize,
 * modules/base/initializers.py:26) -- tf.nn.embedding_lookup, basic_model.py:89-94,106-121.
 * out is [n, out_ld]; columns [dim, out_ld) are zero-filled. */
int oea_gather_rows(const float *table, int32_t dim, int32_t ld, const int32_t *ids, int64_t n,
                    int32_t normalize, float *out, int32_t out_ld, void *stream);
/* in place: table[r] = l2_normalize(table[r]) for all rows (sklearn normalize semantics when
 * sk != 0: zero rows stay zero; TF semantics otherwise: x*rsqrt(max(ss,1e-12))) */
int oea_normalize_rows(float *table, int64_t rows, int32_t dim, int32_t ld, int32_t sk, void *stream);
int oea_fill_f32(float *p, int64_t n, float value, void *stream);
/* device <-> host copies ordered on `stream`, complete on return (staging of oea_comm_init_callbacks hosts) */
int oea_copy_to_host(const void *dev, void *host, size_t bytes, void *stream);
int oea_copy_from_host(void *dev, const void *host, size_t bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Translational step -- replaces one session.run([triple_loss, triple_optimizer]) of
 * BasicModel.launch_triple_training_1epo (basic_model.py:222-232): gather
 * (basic_model.py:89-94) -> l2_normalize (initializers.py:26) -> loss (modules/base/losses.py:
 * 15-73, approaches/bootea.py:197) -> gradient -> duplicate rows summed -> optimizer
 * (modules/base/optimizers.py:4-20).
 * ------------------------------------------------------------------------------------- */
enum { OEA_LOSS_MARGIN = 0, OEA_LOSS_LIMITED = 1, OEA_LOSS_LOGISTIC = 2, OEA_LOSS_POSITIVE = 3,
       OEA_LOSS_ALIGN = 4 };
enum { OEA_OPT_SGD = 0, OEA_OPT_ADAGRAD = 1, OEA_OPT_ADAM = 2, OEA_OPT_ADADELTA = 3 };
enum { OEA_SCORE_TRANSE = 0, OEA_SCORE_TRANSH = 1, OEA_SCORE_TRANSD = 2 };

typedef struct oea_step_cfg {
    int32_t loss_kind;   /* OEA_LOSS_* */
    int32_t l1;          /* 1: args.loss_norm == 'L1'; 0: 'L2' (squared, no sqrt) */
    float margin;        /* margin-based: args.margin */
    float pos_margin;    /* limited: args.pos_margin */
    float neg_margin;    /* limited: args.neg_margin */
    float balance;       /* limited: args.neg_margin_balance */
    int32_t ent_l2_norm; /* args.ent_l2_norm */
    int32_t rel_l2_norm; /* args.rel_l2_norm */
    int32_t opt_kind;    /* OEA_OPT_* (args.optimizer) */
    float lr;            /* args.learning_rate */
    int32_t neg_group_k; /* 0: neg is an arbitrary list (reference order: python set order, batch.py:118).
                            k > 0: n_neg == n_pos*k and neg[p*k .. p*k+k) are the corruptions of pos p as
                            oea_sample_negatives writes them -> one workgroup-lane group scores a positive
                            with its negatives (fewer row reads / atomics; identical arithmetic per triple,
                            entries that are not corruptions of pos p are still scored correctly). */
    int32_t score_kind;  /* OEA_SCORE_TRANSE: s = |h + r - t|;  OEA_SCORE_TRANSH (approaches/bootea_transh.py:58-96):
                            h, t projected on the relation's hyperplane first, h' = h - (h.n) n with
                            n = l2_normalize(l2_normalize(normal[r])) -- also models/trans/transh.py:16-51 (margin
                            pairs, free negative lists).  OEA_SCORE_TRANSD (models/trans/transd.py:16-57):
                            h' = l2_normalize(h + (h.hp) rp) with the transfer vectors hp = ent[ent_transfer_base + h],
                            rp = rel[rel_transfer_base + r] stored in the same tables (below). */
    float *normal;       /* TransH: [n_rel, ld] normal_vector table (trained in place), else NULL */
    float *normal_acc;   /* TransH + Adagrad: its accumulator, else NULL */
    int32_t ent_transfer_base; /* TransD: `ent` has 2*base rows, [0, base) = ent_embeds, [base, 2 base) = ent_transfer */
    int32_t rel_transfer_base; /* TransD: `rel` has 2*base rows, [0, base) = rel_embeds, [base, 2 base) = rel_transfer;
                                  triple ids stay in [0, base); both halves share the l2_norm flag and the optimiser
                                  (transd.py:16-24), so scratch, exchange and apply see ordinary rows */
    /* OEA_OPT_ADAM / OEA_OPT_ADADELTA (optimizers.py:13-16; tf.train defaults): the update is DENSE -- the tables are
     * l2_normalize(variable), the gather gradient comes back through it as a dense tensor -- so every row moves every
     * step.  ent_acc / rel_acc then hold [2, rows, ld]: Adam (m, v) zeros; Adadelta (accum, accum_update) zeros. */
    float beta1;         /* Adam beta1 = 0.9;  Adadelta rho = 0.95 */
    float beta2;         /* Adam beta2 = 0.999 */
    float eps;           /* 1e-8 */
    int32_t opt_t;       /* Adam: 1-based step count of THIS optimiser instance */
} oea_step_cfg;

/* Workspace owned by the caller, sized by oea_step_workspace_bytes(); must be zero-initialised
 * once (hipMemset) before first use; the step leaves it zeroed again. */
size_t oea_step_workspace_bytes(int64_t n_ent, int64_t n_rel, int32_t ld);

/* One optimiser step.  pos/neg: int32 [n,3].  For OEA_LOSS_MARGIN n_neg must equal n_pos
 * (pairs aligned, losses.py:26); neg may be NULL when n_neg == 0 (positive / align losses).
 * ent_acc / rel_acc: Adagrad accumulators (same shape as the tables, initial value 0.1 =
 * tf.train.AdagradOptimizer default), ignored for SGD; Adam / Adadelta: [2, rows, ld] (see oea_step_cfg).
 * loss_accum: device double; the batch loss (sum over the batch, as in the reference) is
 * ADDED to it, so an epoch's loss is read back once (basic_model.py:231-233). */
int oea_triple_step(float *ent, float *ent_acc, int64_t n_ent, float *rel, float *rel_acc,
                    int64_t n_rel, int32_t dim, int32_t ld, const int32_t *pos, int64_t n_pos,
                    const int32_t *neg, int64_t n_neg, const oea_step_cfg *cfg, void *workspace,
                    double *loss_accum, void *stream);

/* The same step split at its one exchange point, for entity-table data parallelism
 * (no reference counterpart: the reference is single-device).  OEA_PHASE_GRAD only fills the
 * gradient scratch + touched flags (the first oea_step_exchange_floats() floats of the
 * workspace, one contiguous fp32 region that the host sums across ranks with ONE RCCL
 * all-reduce); OEA_PHASE_APPLY then runs the optimiser on every rank, so the replicas stay
 * bit-identical.  n_pos / n_neg must be repeated unchanged in the APPLY call. */
enum { OEA_PHASE_BOTH = 0, OEA_PHASE_GRAD = 1, OEA_PHASE_APPLY = 2 };
size_t oea_step_exchange_floats(int64_t n_ent, int64_t n_rel, int32_t ld);
/* Element type of the gradient scratch, the touched flags and every buffer of the partition protocol that carries them
 * (`send`, `own`, `rel_x` below): 4 = fp32 accumulated with hardware fp32 atomics (libopenea_hip.so); 8 = int64 FIXED POINT
 * with 32 fractional bits accumulated with 64-bit integer atomics (libopenea_hip_det.so, the same sources built with
 * -DOEA_DET_SCRATCH): integer sums do not depend on the order of the atomics, so a job gives the same bits run to run and
 * for any number of ranks (the collectives then sum int64: OEA_COMM_I64).  oea_step_exchange_floats counts ELEMENTS of this
 * type. */
int32_t oea_step_scratch_elem_bytes(void);
int oea_triple_step_phase(float *ent, float *ent_acc, int64_t n_ent, float *rel, float *rel_acc,
                          int64_t n_rel, int32_t dim, int32_t ld, const int32_t *pos, int64_t n_pos,
                          const int32_t *neg, int64_t n_neg, const oea_step_cfg *cfg, void *workspace,
                          double *loss_accum, int32_t phase, void *stream);

/* work items of the scoring kernel of a step with n_pos positives and n_neg negatives under `cfg` (= the n_items oea_part_apply is
 * told, which decides how many loss partials it adds up): n_pos when the negatives ride with their positives, n_pos + n_neg else. */
int64_t oea_step_items(const oea_step_cfg *cfg, int64_t n_pos, int64_t n_neg);

/* Entity-id partitioning of the same step across `world` processes (one per GPU): owner of entity row id = id mod world
 * (BASELINE.json north_star; SURVEY 8e: ids are degree-ordered, contiguous ranges would put every hub on rank 0).  Every rank
 * keeps a full read copy of the entity table and the optimiser state of ITS rows only (acc_own [rows_per_rank, ld]).
 *   oea_triple_step_phase(..., OEA_PHASE_GRAD)        local gradients into the workspace scratch
 *   oea_part_pack      scratch -> `send` in owner-major order: world chunks of rpr*(ld+1) floats (rpr rows, then their
 *                      touched flags; rpr = oea_part_rows_per_rank), scratch cleared on the way; relation gradients + flags
 *                      -> rel_x [n_rel*(ld+1)]
 *   reduce-scatter of `send` over the ranks (chunk r to rank r: oea_comm_reduce_scatter_f32 / torch.distributed) -> `own`;
 *   all-reduce of rel_x (relations are few: replicated, every rank applies the same update)
 *   oea_part_apply     optimiser on the owned rows (in place in the natural-order table) + relation rows; the owned rows
 *                      after the update also go to `upd` [rpr, ld]; adds the step's loss (n_items = work items of the GRAD call:
 *                      n_pos for grouped negatives / margin pairs, else n_pos + n_neg)
 *   all-gather of `upd` -> `all` [world][rpr][ld]
 *   oea_part_unpack    the other ranks' rows into the local read copy
 * SGD / Adagrad, TransE score.  Result = the single-process step on the concatenated batch. */
int64_t oea_part_rows_per_rank(int64_t n_ent, int32_t world);
size_t oea_part_send_floats(int64_t n_ent, int32_t ld, int32_t world);
int oea_part_pack(void *workspace, int64_t n_ent, int64_t n_rel, int32_t ld, int32_t world, void *send, void *rel_x,
                  void *stream);
int oea_part_apply(float *ent, float *acc_own, int64_t n_ent, float *rel, float *rel_acc, int64_t n_rel, int32_t ld,
                   int32_t world, int32_t rank, void *own, void *rel_x, float *upd, const oea_step_cfg *cfg, void *workspace,
                   int64_t n_items, double *loss_accum, void *stream);
int oea_part_unpack(float *ent, int64_t n_ent, int32_t ld, int32_t world, int32_t rank, const float *all, void *stream);
/* TransH under the entity-id partition (approaches/bootea_transh.py:58-96): the normal-vector table is relation-sized and
 * replicated.  After the GRAD phase its gradient scratch (copy 0) and touched flags -- [n_rel, ld] and [n_rel] floats at the
 * byte offsets oea_step_normal_scratch reports inside the step workspace -- are summed over the ranks (two small all-reduces),
 * then every rank runs oea_step_apply_normals (the optimiser on the touched rows of cfg->normal, state cfg->normal_acc). */
int oea_step_normal_scratch(int64_t n_ent, int64_t n_rel, int32_t ld, int64_t *grad_offset_bytes, int64_t *touched_offset_bytes);
int oea_step_apply_normals(int64_t n_ent, int64_t n_rel, int32_t ld, const oea_step_cfg *cfg, void *workspace, void *stream);


/* Add externally computed gradients w.r.t. the (normalised) entity rows `ids` into the step's
 * gradient scratch: grad[ids[i]] += src[i].  Followed by oea_triple_step_phase(...,
 * n_pos = n_neg = 0, OEA_PHASE_APPLY) this runs the optimiser for losses that are not
 * translational -- MTransE's mapping loss alpha*(sum|e2 - e1 M|^2 + |M M^T - I|^2)
 * (modules/base/mapping.py:9-19, modules/base/losses.py:76-80), whose d x d GEMMs are plain
 * library GEMMs on the host side. */
int oea_step_scatter_ent_rows(void *workspace, int64_t n_ent, int64_t n_rel, int32_t ld, const int32_t *ids,
                              int64_t n, const float *src, int32_t src_ld, void *stream);

/* ---------------------------------------------------------------------------------------
 * RotatE step in fp64 -- replaces session.run([triple_loss, triple_optimizer]) and
 * session.run([alignment_loss, alignment_optimizer]) of BootEA_RotatE (approaches/bootea_rotate.py:50-109,148-158,
 * 193-203): variables re_ent_embeds / im_ent_embeds / rel_embeds are tf.float64 (bootea_rotate.py:50-57),
 *   theta = l2n?(rel)[r] * phase_scale,  (a, b) = (h_re + i h_im) e^{i theta} - (t_re + i t_im),  dist = sum_d |(a, b)_d|,
 *   loss = sum softplus(dist+ - gamma) + sum softplus(gamma - dist-)        (= -sum log sigmoid(score), :59-81)
 * and TF's optimiser semantics (optimizers.py:4-20): Adam moves EVERY row every step.  The plain RotatE
 * (models/semantic/rotate.py:74-82) divides the negative half by args.neg_triple_num: cfg->neg_loss_div = k > 1 multiplies every
 * negative triple's loss term and its gradients by 1.0 / k; 0 and 1 leave the negatives undivided (BootEA_RotatE, the same bits as
 * before the field had a meaning); a negative value is OEA_EINVAL before anything is launched.
 * ent: [2 n_ent, ld] doubles, rows [0, n_ent) = re_ent_embeds, [n_ent, 2 n_ent) = im_ent_embeds; rel: [n_rel, ld].
 * ent_state / rel_state: Adagrad accumulator [rows, ld] (initial 0.1), or Adam m then v [2, rows, ld] (zeros), NULL for SGD.
 * neg == NULL / n_neg == 0: the positive half alone (alignment loss).  neg_group_k as in oea_step_cfg.
 * phase: OEA_PHASE_*; the exchanged prefix of the workspace is oea_rotate_exchange_doubles() doubles.
 * workspace: oea_rotate_workspace_bytes(), zeroed once; the step leaves it zeroed. ------------------------------- */
typedef struct oea_rotate_cfg {
    double gamma;        /* args.gamma */
    double phase_scale;  /* pi / embedding_range, embedding_range = (gamma + 2.0) / dim  (bootea_rotate.py:29-33,90) */
    double lr;           /* args.learning_rate */
    double beta1, beta2, eps; /* Adam: 0.9, 0.999, 1e-8 (tf.train.AdamOptimizer defaults) */
    int64_t t;           /* Adam: 1-based step count of THIS optimiser instance */
    int32_t ent_l2_norm; /* args.ent_l2_norm (both entity tables) */
    int32_t rel_l2_norm; /* args.rel_l2_norm */
    int32_t opt_kind;    /* OEA_OPT_* */
    int32_t neg_loss_div; /* 0, 1: sum of the negatives' terms; k > 1: that sum / k (rotate.py:81, k = args.neg_triple_num) */
} oea_rotate_cfg;
size_t oea_rotate_workspace_bytes(int64_t n_ent, int64_t n_rel, int32_t ld);
size_t oea_rotate_exchange_doubles(int64_t n_ent, int64_t n_rel, int32_t ld);
int oea_rotate_step(double *ent, double *ent_state, int64_t n_ent, double *rel, double *rel_state, int64_t n_rel,
                    int32_t dim, int32_t ld, const int32_t *pos, int64_t n_pos, const int32_t *neg, int64_t n_neg,
                    int32_t neg_group_k, const oea_rotate_cfg *cfg, void *workspace, double *loss_accum, int32_t phase,
                    void *stream);
/* out[i, 0:dim] = (float)( l2n?( part(re[ids[i]]) + part(im[ids[i]]) ) ), part = l2_normalize when part_norm: the
 * embeddings that evaluation, bootstrapping and the neighbour search of BootEA_RotatE read
 * (bootea_rotate.py:111-146,160-167: `re_ent_embeds + im_ent_embeds`, normalised again when sum_norm).
 * ids == NULL: rows 0..n-1.  out is fp32 [n, out_ld], pad columns zero -- the evaluation kernels are fp32. */
int oea_rotate_lookup(const double *ent, int64_t n_ent, int32_t dim, int32_t ld, const int32_t *ids, int64_t n,
                      int32_t part_norm, int32_t sum_norm, float *out, int32_t out_ld, void *stream);

/* MTransE's mapping step, fused (modules/base/mapping.py:9-19, losses.py:76-80, approaches/mtranse.py:84-96):
 *   loss = alpha * (sum_n ||e2_n - e1_n M||^2 + ||M M^T - I||_F^2),  e = l2_normalize(ent)[ids] (if ent_l2_norm).
 * M [dim, dim] row-major is updated in place (Adagrad with M_acc, or SGD); the gradients w.r.t. the NORMALISED
 * entity rows are added into ent_grad [n_ent, ld] / ent_touched -- the step workspace's scratch, see
 * oea_step_entity_scratch() -- so that oea_triple_step_phase(..., n_pos = 0, OEA_PHASE_APPLY) finishes the step.
 * work: oea_mapping_workspace_floats(n, ld, dim) floats.  loss_accum += the batch loss. */
size_t oea_mapping_workspace_floats(int64_t n_links, int32_t ld, int32_t dim);
int oea_mapping_step(const float *ent, int32_t ld, int32_t dim, int32_t ent_l2_norm, const int32_t *ids1,
                     const int32_t *ids2, int64_t n, float *M, float *M_acc, float alpha, float lr, int32_t opt_kind,
                     void *ent_grad, void *ent_touched, float *work, double *loss_accum, void *stream);
/* A whole mapping epoch (approaches/mtranse.py:84-96) enqueued by ONE call: `steps` x (oea_mapping_step on the step's n links +
 * the apply phase of the step engine with `cfg`).  batches: device int32 [steps, 2, n].  Single process only (a data-parallel
 * job exchanges the scratch between the two halves of every step). */
int oea_mapping_epoch(float *ent, float *ent_acc, int64_t n_ent, float *rel, float *rel_acc, int64_t n_rel, int32_t dim,
                      int32_t ld, int32_t ent_l2_norm, const int32_t *batches, int32_t steps, int64_t n, float *M, float *M_acc,
                      float alpha, float lr, int32_t opt_kind, const oea_step_cfg *cfg, void *workspace, float *work,
                      double *mapping_loss_accum, double *step_loss_accum, void *stream);
/* SEA's mapping step, fused (approaches/sea.py:73-98,129-145): two dim x dim matrices, a supervised loss in both directions on
 * the labelled links (l1[i], l2[i]) and a cycle loss in both directions on the unlabelled links (u1[j], u2[j]):
 *   E = l2_normalize(ent, 1) (if cfg->ent_l2_norm);  L1 = E[l1], L2 = E[l2], U1 = E[u1], U2 = E[u2]
 *   loss = alpha_1 (|L2 - gl2n(L1 M1)|^2 + |L1 - gl2n(L2 M2)|^2) + alpha_2 (|U1 - gl2n(U1 M1 M2)|^2 + |U2 - gl2n(U2 M2 M1)|^2)
 * where gl2n is tf.nn.l2_normalize WITHOUT an axis, as the reference calls it: the whole [n, dim] block divided by
 * sqrt(max(sum of all its squares, 1e-12)).  M1 / M2 [dim, dim] row-major are updated in place by SGD or Adam (cfg->opt_kind, lr,
 * beta1, beta2, eps, opt_t; M_state = Adam's [m1; v1; m2; v2], 4 dim^2 zeros at the start, NULL for SGD); every block scalar and
 * every element of the matrix gradients is summed in a fixed order without float atomics: M1 / M2 have the same bits run to run.
 * The gradients w.r.t. the NORMALISED entity rows are added into ent_grad / ent_touched (oea_step_entity_scratch), an entity that
 * occurs several times summed, so that oea_triple_step_phase(..., n_pos = 0, OEA_PHASE_APPLY) with the same cfg finishes the step.
 * n_l == 0 or n_u == 0 alone is legal (that half contributes nothing).  Adagrad / Adadelta, dim > 128: OEA_EUNSUPPORTED;
 * ld % 4 != 0, n_l == n_u == 0: OEA_EINVAL -- both before anything is launched.  work: oea_sea_mapping_workspace_floats(n_l, n_u,
 * ld, dim) floats, 16-byte aligned, no initialisation needed.  loss_accum += the batch loss. */
size_t oea_sea_mapping_workspace_floats(int64_t n_l, int64_t n_u, int32_t ld, int32_t dim);
int oea_sea_mapping_step(const float *ent, int32_t ld, int32_t dim, const int32_t *ids_l1, const int32_t *ids_l2, int64_t n_l,
                         const int32_t *ids_u1, const int32_t *ids_u2, int64_t n_u, float *M1, float *M2, float *M_state,
                         float alpha_1, float alpha_2, const oea_step_cfg *cfg, void *ent_grad, void *ent_touched, float *work,
                         double *loss_accum, void *stream);
/* A whole mapping epoch of SEA enqueued by ONE call: `steps` x (oea_sea_mapping_step + the apply phase of the step engine with
 * `cfg`, whose opt_t counts up from cfg->opt_t).  batches: device int32 [steps][l1 (n_l) | l2 (n_l) | u1 (n_u) | u2 (n_u)].
 * ent_acc / rel_acc: the mapping optimiser's own state ([2, rows, ld] for Adam).  Single process only (the block scalars of a
 * data-parallel job would need an all-reduce between the phases of every step). */
int oea_sea_mapping_epoch(float *ent, float *ent_acc, int64_t n_ent, float *rel, float *rel_acc, int64_t n_rel, int32_t dim,
                          int32_t ld, const int32_t *batches, int32_t steps, int64_t n_l, int64_t n_u, float *M1, float *M2,
                          float *M_state, float alpha_1, float alpha_2, const oea_step_cfg *cfg, void *workspace, float *work,
                          double *mapping_loss_accum, double *step_loss_accum, void *stream);
/* TransR's step (models/trans/transr.py:13-50): x = l2n(ent)[e], y' = l2n(M_r x) with M_r = rel_matrix[r] as a row-major
 * dim x dim matrix, for h and t of the positive and of the negative (each with its own triple's relation), r = l2n(rel)[r]
 * unprojected, loss = sum relu(margin + |h'+r-t'|^2 - |nh'+nr-nt'|^2) over the pairs (pos i, neg i).  The projections run
 * grouped by relation on the fp32 matrix cores (M_r staged once per tile of <= 64 items).  rel_matrix [n_rel, dim*dim] (and
 * rel_matrix_acc: Adagrad, initial 0.1) is updated inside the call, relations absent from the batch untouched and the tiles of a
 * relation summed in a fixed order; the entity / relation row gradients go into the step workspace's scratch and the call ends
 * with oea_triple_step_phase(..., n_pos = 0, OEA_PHASE_APPLY).  cfg: score_kind OEA_SCORE_TRANSE, loss_kind OEA_LOSS_MARGIN,
 * l1 = 0, opt_kind SGD or Adagrad; n_neg == n_pos; dim <= 128 (OEA_EUNSUPPORTED above).  step_workspace: as for
 * oea_triple_step; transr_workspace: oea_transr_workspace_bytes(n_ent, n_rel, dim, max_pos) bytes for n_pos <= max_pos (no
 * initialisation needed).  loss_accum += the batch loss. */
size_t oea_transr_workspace_bytes(int64_t n_ent, int64_t n_rel, int32_t dim, int64_t max_pos);
int oea_transr_step(float *ent, float *ent_acc, int64_t n_ent, float *rel, float *rel_acc, int64_t n_rel, float *rel_matrix,
                    float *rel_matrix_acc, int32_t dim, int32_t ld, const int32_t *pos, int64_t n_pos, const int32_t *neg,
                    int64_t n_neg, const oea_step_cfg *cfg, void *step_workspace, void *transr_workspace, double *loss_accum,
                    void *stream);
/* The semantic-matching models' step (models/semantic/{hole,simple,distmult}.py), one wave per positive and its k negatives:
 *   OEA_SEMANTIC_HOLE    u = l2n(ent)[e], rh = l2n(l2n(rel)[r]) (normalised twice, hole.py:57), c = ccorr(uh, ut) with
 *                        c[k] = sum_i uh[i] ut[(i + k) mod dim], score = -sigmoid(rh . c),
 *                        loss = sum_p relu(margin + score_p - mean_j score_{p,j}) (hole.py:41-86);
 *   OEA_SEMANTIC_SIMPLE  ent = [H; T] (2E rows), rel = [R1; R2] (2R rows), each row l2-normalised, triple ids in [0, E) / [0, R),
 *                        score = (l2n(H[h] o R1[r]) . T[t] + l2n(H[t] o R2[r]) . T[h]) / 2,
 *                        loss = sum_pos softplus(-score) + sum_neg softplus(score) (simple.py:39-88);
 *   OEA_SEMANTIC_DISTMULT u = l2n?(ent)[e], w = l2n?(rel)[r] (by cfg->ent_l2_norm / rel_l2_norm), score = sum_d uh[d] w[d] ut[d],
 *                        loss = MEAN over the N = n_pos + n_neg labelled triples of softplus(-y score), y = +1 for pos, -1 for neg
 *                        (distmult.py:43-59, batch.py:generate_triple_label_batch); tables not stacked.
 * neg[p k .. p k + k) are the k = cfg->neg_group_k >= 1 corruptions of pos p (the device sampler's layout), n_neg == k n_pos.
 * cfg: margin (HolE), neg_group_k, ent_l2_norm / rel_l2_norm, opt_kind SGD or Adagrad, lr; score_kind stays OEA_SCORE_TRANSE and
 * loss_kind is not read (the model brings its own).  The row gradients go into the step workspace's scratch (entity rows, relation
 * copy 0; a row that a positive shares with its negatives as one summed row) and the call ends with
 * oea_triple_step_phase(..., n_pos = 0, OEA_PHASE_APPLY); step_workspace: as for oea_triple_step with (n_ent, n_rel) = the table
 * rows.  Unknown model, Adam / Adadelta, dim > 128: OEA_EUNSUPPORTED; n_neg != k n_pos, ld % 4 != 0: OEA_EINVAL -- both before
 * anything is launched.  loss_accum += the batch loss (DistMult: the batch mean). */
enum { OEA_SEMANTIC_HOLE = 0, OEA_SEMANTIC_SIMPLE = 1, OEA_SEMANTIC_DISTMULT = 2 };
int oea_semantic_step(int32_t model, float *ent, float *ent_acc, int64_t n_ent, float *rel, float *rel_acc, int64_t n_rel,
                      int32_t dim, int32_t ld, const int32_t *pos, int64_t n_pos, const int32_t *neg, int64_t n_neg,
                      const oea_step_cfg *cfg, void *step_workspace, double *loss_accum, void *stream);
/* JAPE's triple step (approaches/jape.py:59-84), one wave per positive and its k = cfg->neg_group_k negatives as above:
 *   u = l2n?(ent)[e], w = l2n?(rel)[r] (by cfg->ent_l2_norm / rel_l2_norm), score = |uh + w - ut|^2,
 *   loss = sum_pos score - neg_alpha sum_neg score   (a negative weight on the negatives and no hinge: none of OEA_LOSS_*).
 * neg, cfg, step_workspace and the closing oea_triple_step_phase(..., n_pos = 0, OEA_PHASE_APPLY) as for oea_semantic_step.
 * Adam / Adadelta, dim > 128: OEA_EUNSUPPORTED; n_neg != k n_pos, ld % 4 != 0, neg_alpha < 0 or NaN: OEA_EINVAL -- both before
 * anything is launched.  loss_accum += the batch SUM (it may be negative). */
int oea_jape_step(float *ent, float *ent_acc, int64_t n_ent, float *rel, float *rel_acc, int64_t n_rel, int32_t dim, int32_t ld,
                  const int32_t *pos, int64_t n_pos, const int32_t *neg, int64_t n_neg, float neg_alpha, const oea_step_cfg *cfg,
                  void *step_workspace, double *loss_accum, void *stream);
/* ---- MultiKE (approaches/multi_ke.py; csrc/multike_step.hip) ------------------------------------------------------------------
 * oea_multike_cnn_step: the attribute CNN (multi_ke.py:154-176) on a batch of n positives (entity, attribute, literal), int32
 * [n, 3].  attr [n_attr, ld] is read raw, lit [n_lit, ld] is constant, a net's entity table [n_ent, ld] is read through the row
 * normalisation when ent_l2_norm is set.  With c = 1 / sqrt(1 + 1e-3):
 *   x = (a ; v) gamma c + beta;  z1 = tanh(conv(x, K1[2,4,1,2]) + b1);  z2 = tanh(conv(z1, K2[2,4,2,2]) + b2)   ('same': rows padded
 *   (0, 1), columns (1, 2));  n = z2 / max(|z2| along the width, 1e-6);  t = tanh(flat(n) . W[4 dim, ld] + bd), flat in the order
 *   (row, column, channel);  y = t / max(|t|_F over the whole batch, 1e-6);  loss = factor sum_b w_b softplus(|h_b - y_b|^2),
 *   w_b = attr_weight[attribute of b] for a weighted net, 1 otherwise.
 * n_nets = 1 or 2 nets share the batch; p = gamma [dim], beta [dim], K1 [16], b1 [2], K2 [32], b2 [2], W [4 dim, ld], bd [dim].
 * The gradients w.r.t. the normalised entity rows go into the entity rows of the net's own step workspace (oea_step_workspace_bytes
 * (n_ent, n_rel_ws, ld)), those w.r.t. the attribute rows of ALL nets into the relation rows of net 0's (n_rel_ws == n_attr there):
 * oea_triple_step_phase(..., n_pos = 0, OEA_PHASE_APPLY) on each finishes the step.  OEA_PHASE_GRAD leaves the eight parameter
 * gradients of net k readable through oea_multike_cnn_grads (same order; W with stride ld); OEA_PHASE_BOTH also runs SGD with lr on
 * the parameters.  Everything summed over the batch is an fp64 partial per workgroup added in a fixed order.
 * workspace: oea_multike_cnn_workspace_bytes(dim, ld, max_n) bytes for n <= max_n, no initialisation needed.  loss_accum += the loss
 * of all nets.  dim > 128: OEA_EUNSUPPORTED; ld % 4 != 0, n < 1, n > max_n, a null pointer, OEA_PHASE_APPLY: OEA_EINVAL -- both before
 * anything is launched.  ids are not checked on the device.  One GPU. */
typedef struct oea_multike_net {
    float *p[8];
    const float *ent;
    void *step_workspace;
    int64_t n_rel_ws;
    int32_t weighted;
    int32_t ent_l2_norm;
    float factor;
} oea_multike_net;
size_t oea_multike_cnn_workspace_bytes(int32_t dim, int32_t ld, int64_t max_n);
int oea_multike_cnn_grads(void *workspace, int32_t dim, int32_t ld, int64_t max_n, int32_t net, void **grads);
int oea_multike_cnn_step(const oea_multike_net *nets, int32_t n_nets, int64_t n_ent, const float *attr, int64_t n_attr,
                         const float *lit, int64_t n_lit, int32_t dim, int32_t ld, const int32_t *batch, int64_t n,
                         const float *attr_weight, float lr, void *workspace, int64_t max_n, double *loss_accum, int32_t phase,
                         void *stream);
/* oea_multike_rows: the row-wise terms of MultiKE's other views, one wave per item, gradients w.r.t. the (normalised) rows into
 * the step workspaces ws_a (n_ent, n_rel_a) of table_a and ws_b (n_ent, n_rel_b) of table_b:
 *   OEA_MULTIKE_ROWS_CROSS  coef |A[h] + rel[r] - B[t]|^2                         items int32 [n, 3]
 *   OEA_MULTIKE_ROWS_PULL   coef |A[e] - B[e]|^2                                  items int32 [n]; ws_b NULL: B is constant
 *   OEA_MULTIKE_ROWS_WSOFT  coef rel_weight[r] softplus(|A[h] + rel[r] - B[t]|^2)  items int32 [n, 3]
 * The relation rows' gradients go into the relation rows of ws_a (rel_side 0) or ws_b (rel_side 1).  An id that repeats counts as
 * often.  loss_accum += the sum.  n == 0 launches nothing.  dim > 128: OEA_EUNSUPPORTED; ld % 4 != 0, a null pointer: OEA_EINVAL. */
enum { OEA_MULTIKE_ROWS_CROSS = 0, OEA_MULTIKE_ROWS_PULL = 1, OEA_MULTIKE_ROWS_WSOFT = 2 };
int oea_multike_rows(int32_t kind, const float *table_a, void *ws_a, int64_t n_rel_a, int32_t a_l2_norm, const float *table_b,
                     void *ws_b, int64_t n_rel_b, int32_t b_l2_norm, const float *rel, int32_t rel_l2_norm, int64_t n_ent,
                     int32_t rel_side, int32_t dim, int32_t ld, const int32_t *items, int64_t n, const float *rel_weight, float coef,
                     double *loss_accum, void *stream);
/* AttrE's character step (approaches/attre.py:88-109, 166-187; csrc/attre_step.hip), one wave per positive (e, a, v) and its
 * k = cfg->neg_group_k head-corrupted negatives (e', a, v), e' = neg_heads[p k .. p k + k):
 *   ue = l2n?(ent_ce)[e], wa = l2n?(attr)[a], v = sum_p w_p l2n?(chars)[value_chars[v, p]], w_p = sum_{m = p + 1 .. L} 1 / m,
 *   score = |ue + wa - v|^2 (cfg->l1: |.|_1), loss = cfg->loss_kind, one of margin-based (k == 1), limited, logistic (losses.py).
 * ent_ce is the step engine's entity table and attr its relation table: cfg->ent_l2_norm / rel_l2_norm (= attr_l2_norm) / opt_kind
 * (SGD or Adagrad) / lr, step_workspace as for oea_triple_step with (n_ent, n_attr), and the call ends with
 * oea_triple_step_phase(..., n_pos = 0, OEA_PHASE_APPLY).  The character table [n_chars, ld] (normalised by char_l2_norm) gets its
 * gradient without row atomics from every positive: the scoring kernel stores dL/dv per positive, a second kernel sums
 * w_i dL/dv[p] per character -- char_path 0: in LDS slabs of [n_chars, ld] while n_chars <= oea_attre_lds_chars(ld), n_slabs
 * workgroups (0: one per 16 positives, at most one per CU; never above 512) each writing a partial; else by atomic row adds into one dense buffer; 1 / 2
 * force the LDS / the atomic path -- and a closing kernel adds the partials in a fixed order, goes back through the normalisation
 * (clamp 1e-12) and runs SGD or Adagrad (char_acc, initial value 0.1) on the n_chars rows.  value_chars int32 [n_values, literal_len]
 * (id 0: padding, a trained row); pos int32 [n_pos, 3] = (entity, attribute, row of value_chars).  char_workspace:
 * oea_attre_char_workspace_bytes(n_chars, ld, n_pos) bytes or more, no initial value.  A check kernel runs first: a character id
 * outside [0, n_chars) sets bit 1 of *err_flag (device int32, zeroed by the caller), a value, entity or attribute id outside its
 * table bit 2, and with the flag set nothing is written.  loss_accum += the batch sum.  Adam / Adadelta, dim > 128:
 * OEA_EUNSUPPORTED; n_neg != k n_pos, margin-based with k != 1, another loss_kind, ld % 4 != 0, literal_len outside 1..32, char_path 1
 * with a slab that does not fit, a workspace too small, a null pointer: OEA_EINVAL -- both before anything is launched. */
int64_t oea_attre_lds_chars(int32_t ld);
size_t oea_attre_char_workspace_bytes(int64_t n_chars, int32_t ld, int64_t max_pos);
int oea_attre_char_step(float *ent_ce, float *ent_acc, int64_t n_ent, float *attr, float *attr_acc, int64_t n_attr, float *chars,
                        float *char_acc, int64_t n_chars, int32_t dim, int32_t ld, const int32_t *value_chars, int64_t n_values,
                        int32_t literal_len, const int32_t *pos, int64_t n_pos, const int32_t *neg_heads, int64_t n_neg,
                        int32_t char_l2_norm, int32_t char_path, int32_t n_slabs, const oea_step_cfg *cfg, void *step_workspace,
                        void *char_workspace, size_t char_workspace_bytes, int32_t *err_flag, double *loss_accum, void *stream);
/* AttrE's negatives (generate_neg_attribute_triples, batch.py:187-199): only the head is corrupted, and with a value id of its own
 * per triple the reference's redraw rejects exactly e' == e.  out[p k + s] = entity_list[j], j uniform over the list's positions
 * without ent_pos[head of p] (ent_pos int32 [n_ent]: position in the side's list, -1 elsewhere), from Philox4x32-10 with counter
 * (p + pos_offset, step, 0, s) keyed by the seed: a pure function of (seed, step, position).  Positives [0, n_split) draw from side
 * 0, the rest from side 1.  out: device int32 [n_pos k].  A side in use with n_ent_list < 2 (the reference would spin), k < 1, a
 * null pointer: OEA_EINVAL before any launch. */
int oea_attre_sample_heads(const int32_t *pos, int64_t n_pos, int64_t n_split, int32_t k, const int32_t *entity_list0, int32_t n_ent_list0,
                           const int32_t *ent_pos0, const int32_t *entity_list1, int32_t n_ent_list1, const int32_t *ent_pos1,
                           int64_t n_ent, uint64_t seed, uint32_t step, uint32_t pos_offset, int32_t *out, void *stream);
/* `steps` joint steps of AttrE (attre.py:189-191, 221-233) in one pass: loss = sum_e (1 - l2n?(ent)[e] . l2n?(ent_ce)[e]) over the
 * WHOLE entity list in every step, so a wave holds row e of both tables over the steps (SGD, or Adagrad with the two accumulators of
 * this optimiser instance) and stores once; the tables equal `steps` calls with steps = 1 bit for bit.  row_count int32 [n_ent]: how
 * often the list names row e (under the sharing alignment a training pair is one id in both KGs' lists: 2; 0: the row stays), its
 * term and gradient times that; NULL: every row once.  loss_accum: device double [steps], loss_accum[s] += the loss of step s.  Adam / Adadelta, dim > 128: OEA_EUNSUPPORTED; ld % 4 != 0, n_ent < 1, steps < 1, a
 * null pointer: OEA_EINVAL -- both before any launch. */
int oea_attre_joint_epoch(float *ent, float *ent_acc, float *ent_ce, float *ent_ce_acc, const int32_t *row_count, int64_t n_ent, int32_t dim,
                          int32_t ld, int32_t ent_l2_norm, int32_t opt_kind, float lr, int32_t steps, double *loss_accum, void *stream);
/* m distinct elements of [0, n) (random.sample(range(n), m), attr2vec.py:150 / jape.py:134): out[i] = pi(i), i < m, with pi a
 * bijection of [0, n) that is a pure function of (seed, step) -- a 6-round Feistel network over max(2, ceil(log2 n)) bits, cycle
 * walked into [0, n), its round keys from Philox4x32-10(counter = (step lo, step hi, 0x64697374, 0 | 1), key = (seed lo, seed hi))
 * (csrc/sample_distinct.hip).  out: device int32 [m].  One launch, no host read.  n < 1, n >= 2^31, m > n: OEA_EINVAL. */
int oea_sample_distinct(int64_t n, int64_t m, uint64_t seed, uint64_t step, int32_t *out, void *stream);
/* JAPE's thresholded attribute similarity as a CSR (jape.py:147-149: sim_mat[sim_mat < threshold] = 0), never dense beyond one block
 * of rows: for row blocks of block_rows rows of e1, oea_sim_matrix(OEA_METRIC_INNER) into block_buf (block_rows * n2 floats), and the
 * entries >= threshold are kept.  oea_sim_csr_count writes indptr int64 [n1 + 1] (indptr[n1] = nnz, which the caller reads back to
 * allocate); oea_sim_csr_fill, with the same arguments and that indptr, writes col int32 [nnz] (ascending within a row) and val
 * fp32 [nnz] (both at least one element long), and adds to *mismatch (device int32, zeroed by the caller) the number of rows
 * that kept another number of entries than oea_sim_csr_count found: 0 as long as oea_sim_matrix repeats its bits.  A null pointer, n1 < 1, n2 < 1, ld % 4 != 0, a NaN threshold: OEA_EINVAL before any launch. */
int oea_sim_csr_count(const float *e1, int64_t n1, int32_t ld1, const float *e2, int64_t n2, int32_t ld2, int32_t dim, float threshold,
                      int64_t block_rows, float *block_buf, int64_t *indptr, void *stream);
int oea_sim_csr_fill(const float *e1, int64_t n1, int32_t ld1, const float *e2, int64_t n2, int32_t ld2, int32_t dim, float threshold,
                     int64_t block_rows, float *block_buf, const int64_t *indptr, int32_t *col, float *val, int32_t *mismatch,
                     void *stream);
/* JAPE's similarity loss (jape.py:86-95) over that CSR, for the m sampled positions rows[i] into ref1 (one wave per row, fp64):
 *   t = sum_j val_ij l2n(ent)[ref2_ids[col_ij]],   loss_accum += beta sum_i | l2n(ent)[ref1_ids[rows[i]]] - l2n(t) |^2,
 * l2n(v) = v / sqrt(max(|v|^2, 1e-12)), so an empty row gives l2n(0) = 0.  Nothing but loss_accum is written: the reference builds
 * sim_optimizer and never runs it (jape.py:136 fetches self.sim_loss alone).  col / val: non-null also for an empty matrix (they
 * are then not read).  dim > 128: OEA_EUNSUPPORTED; ld % 4 != 0, a null pointer: OEA_EINVAL -- before any launch.  ids are not checked on the device. */
int oea_jape_sim_loss(const float *ent, int64_t n_ent, int32_t dim, int32_t ld, const int32_t *ref1_ids, int64_t n_ref1,
                      const int32_t *ref2_ids, int64_t n_ref2, const int64_t *indptr, const int32_t *col, const float *val,
                      const int32_t *rows, int64_t m, float beta, double *loss_accum, void *stream);

/* ---------------------------------------------------------------------------------------
 * IMUSE's string similarity (approaches/imuse.py:42-66, 195-249; csrc/lcs_sim.hip).  Levenshtein.ratio(a, b) =
 * 2 LCS(a, b) / (|a| + |b|) over code points, 1.0 when both are empty; LCS by the bit-vector recurrence with the pattern's
 * character masks in an LDS table (patterns up to 256 code points), by a wave-wide row DP beyond that.  Integers are exact and the
 * ratio is (double)(2 lcs) / (double)(|a| + |b|): the bits Python gives.
 *
 * STRING POOL (one per KG side, built once on the host): cp int32 [n_cp] = the distinct strings as UTF-32 code points back to back
 * (each in [0, 0x10FFFF]), off int64 [n_str + 1] with off[0] = 0 and off[n_str] = n_cp.  max_len: the caller's bound on the length
 * of any string of either pool.  workspace: oea_lcs_workspace_ints(max_len) int32 of device memory.
 *
 * What the host sees is refused by the return status before any launch: a null pointer, n_str < 1, n_cp < 0, max_len < 0, n < 0,
 * K < 1 or K > 32, n1 < 1, n2 < 1, cap < 1, a NaN threshold -> OEA_EINVAL.  What lies in device memory -- offsets that decrease,
 * do not start at 0 or end at n_cp, a string longer than max_len, an index outside its pool, a row outside [0, n1) -- is found by
 * check kernels that run first on the stream: they set *err_flag (device int32, zeroed by the caller; bit 0 a pool, bit 1 an index)
 * and the compute kernels then write NOTHING.  The caller reads err_flag with the results.  No host synchronisation inside.
 * ------------------------------------------------------------------------------------- */
size_t oea_lcs_workspace_ints(int64_t max_len);
/* pairs int32 [n, 2] = (string of pool 1, string of pool 2) -> lcs int32 [n], ratio fp64 [n].  One wave per pair; the shorter
 * string is the pattern, so only a pair whose SHORTER side exceeds 256 code points takes the row DP. */
int oea_lcs_ratio_pairs(const int32_t *cp1, const int64_t *off1, int64_t n_str1, int64_t n_cp1, const int32_t *cp2, const int64_t *off2,
                        int64_t n_str2, int64_t n_cp2, int64_t max_len, const int32_t *pairs, int64_t n, int32_t *lcs, double *ratio,
                        int32_t *workspace, int32_t *err_flag, void *stream);
/* The records of run_one_ea's walk (imuse.py:47-62), without the n1 x n2 matrix.  K aligned attribute pairs IN THE CALLER'S ORDER;
 * idx1 int32 [K, n1] / idx2 int32 [K, n2]: the value (an index into pool 1 / pool 2) that entity i / j holds for pair k, -1 for
 * none.  For row i and j = 0 .. n2 - 1 in order, in fp64:
 *     s = 0, c = 0;  for k = 0 .. K - 1: if both present: s += ratio(value1, value2), c += 1;   if c > 0: s /= c
 * and (j, s) is a RECORD when s > threshold and s > every earlier s of the row (strictly: a tie is none).
 * rows int32 [n_rows] (NULL: all n1 rows, n_rows == n1) selects the rows; output slot r belongs to rows[r]:
 *     rec_col int32 [n_rows, cap], rec_val fp64 [n_rows, cap]   the first min(count, cap) records of the row, j ascending
 *     rec_cnt int32 [n_rows] = min(count, cap),  overflow int32 [n_rows] = 1 when the row has more than cap records
 * A caller must rerun the rows that overflowed with a larger cap: no record is dropped without the flag.
 * One workgroup per row: the row's K tables are built once and serve the whole walk. */
int oea_attr_sim_records(const int32_t *cp1, const int64_t *off1, int64_t n_str1, int64_t n_cp1, const int32_t *cp2, const int64_t *off2,
                         int64_t n_str2, int64_t n_cp2, int64_t max_len, int32_t K, const int32_t *idx1, int64_t n1,
                         const int32_t *idx2, int64_t n2, double threshold, const int32_t *rows, int64_t n_rows, int32_t cap,
                         int32_t *rec_col, double *rec_val, int32_t *rec_cnt, int32_t *overflow, int32_t *workspace, int32_t *err_flag,
                         void *stream);

/* The candidate sets of n_steps steps in ONE launch, for the steps that are too short to wait for oea_log_uniform_sample's status
 * word (declared with ProjE below; the values here are its values bit for bit): workgroup s writes out_ids[s, :], out_num_tries[s],
 * out_log_q_sampled[s, :] of step step0 + s, and status[s] = 0, or 1 when n_sampled distinct classes did not appear in 64 n_sampled
 * draws (that step's ids are then 0 .. n_sampled - 1 with log Q 0: in bounds, not a sample); the caller reads status once per
 * epoch.  The first-appearance table lives in LDS: n_classes > OEA_LOG_UNIFORM_STEPS_MAX_CLASSES is OEA_EUNSUPPORTED before any
 * launch; n_sampled < 1, n_sampled > n_classes, a null pointer: OEA_EINVAL. */
#define OEA_LOG_UNIFORM_STEPS_MAX_CLASSES 8192
int oea_log_uniform_sample_steps(int64_t n_classes, int64_t n_sampled, uint64_t seed, uint64_t step0, int64_t n_steps,
                                 const double *thresholds, int32_t *out_ids, int64_t *out_num_tries, float *out_log_q_sampled,
                                 int32_t *status, void *stream);
/* Attr2Vec's step (approaches/attr2vec.py:106-124): a skip-gram over attribute pairs under tf.nn.nce_loss and Adagrad.
 *   x_b = l2n(embeds)[in_b], w_c = l2n(nce_weights)[c]; true_b = x_b . w_lab + bias[lab] - log Q(lab), samp_bj = x_b . w_sj + bias[s_j]
 *   - log Q(s_j); loss = mean_b (softplus(-true_b) + sum_j softplus(samp_bj)); log Q as for ProjE (num_true = 1, accidental hits
 *   kept, range_max = n_attr, the labels' at *num_tries).
 * pairs int32 [n_batch, 2] = (input, label); sampled / log_q_sampled [n_sampled] and num_tries as the samplers write them.  The
 * sampled half runs over DISTINCT inputs x candidates, weighted by an input's multiplicity (csrc/attr2vec_step.hip).  phase:
 * OEA_PHASE_GRAD leaves the gradients w.r.t. embeds [n_attr, ld], nce_weights [n_attr, ld], nce_biases [n_attr] (dense fp32, rows
 * the batch did not touch zero) readable through oea_attr2vec_grads; OEA_PHASE_APPLY runs Adagrad (acc += g^2, v -= lr g /
 * sqrt(acc); accumulators start at 0.1) on the rows that received gradient, all others keep their bits.  workspace:
 * oea_attr2vec_workspace_bytes(n_attr, ld, max_sampled) bytes, zeroed once, n_sampled <= max_sampled.  loss_accum += the batch
 * MEAN.  OEA_PHASE_APPLY reads neither the batch nor the candidates: pairs, sampled, log_q_sampled, num_tries may be NULL and
 * n_batch, n_sampled anything there.  dim > 128: OEA_EUNSUPPORTED; ld % 4 != 0, and outside OEA_PHASE_APPLY n_batch < 1, n_sampled
 * < 1 or > n_attr or > max_sampled, a null pointer: OEA_EINVAL -- both before anything is launched.  ids are not checked on the device.  One GPU.
 * oea_attr2vec_epoch: `steps` steps over the device list pairs [n_pairs, 2] in one call with no host round trip: the candidates of
 * all steps by oea_log_uniform_sample_steps(seed, step0) into cand_* ([steps, n_sampled], [steps], [steps, n_sampled], status
 * [steps], which the caller reads afterwards), then per step batch_idx [n_batch] = oea_sample_distinct(n_pairs, n_batch, seed,
 * step0 + s) and the step on pairs[batch_idx].  A step whose status word is not 0 changes nothing (its kernels return at once),
 * so when the caller finds a failed draw the tables hold the other steps' updates only.  steps == 0 does nothing, whatever
 * n_pairs is.  n_attr > OEA_LOG_UNIFORM_STEPS_MAX_CLASSES: OEA_EUNSUPPORTED. */
typedef struct oea_attr2vec_vars {
    float *embeds, *embeds_acc, *nce_weights, *nce_weights_acc, *nce_biases, *nce_biases_acc;
} oea_attr2vec_vars;
size_t oea_attr2vec_workspace_bytes(int64_t n_attr, int32_t ld, int64_t max_sampled);
int oea_attr2vec_grads(void *workspace, int64_t n_attr, int32_t ld, int64_t max_sampled, void **grads);
int oea_attr2vec_step(const oea_attr2vec_vars *vars, int64_t n_attr, int32_t dim, int32_t ld, const int32_t *pairs, int64_t n_batch,
                      const int32_t *sampled, int64_t n_sampled, const float *log_q_sampled, const int64_t *num_tries, float lr,
                      void *workspace, int64_t max_sampled, double *loss_accum, int32_t phase, void *stream);
int oea_attr2vec_epoch(const oea_attr2vec_vars *vars, int64_t n_attr, int32_t dim, int32_t ld, const int32_t *pairs, int64_t n_pairs,
                       int64_t n_batch, int32_t steps, uint64_t seed, uint64_t step0, const double *thresholds, int64_t n_sampled,
                       int32_t *cand_ids, int64_t *cand_tries, float *cand_log_q, int32_t *cand_status, int32_t *batch_idx, float lr,
                       void *workspace, int64_t max_sampled, double *loss_accum, void *stream);
/* addresses of the entity gradient scratch and its touched flags inside a step workspace */
int oea_step_entity_scratch(void *workspace, int64_t n_ent, int64_t n_rel, int32_t ld, void **ent_grad,
                            void **ent_touched);

/* ---- ProjE (models/neural/proje.py) --------------------------------------------------------------------------------------------
 * oea_log_uniform_sample: the candidate sampler of the sampled softmax.  n_sampled DISTINCT classes of [0, n_classes) under the
 * log-uniform law P(c) = (log(c + 2) - log(c + 1)) / log(n_classes + 1), drawn one after another until n_sampled distinct values
 * have appeared; out_ids holds them in the order of first appearance, *out_num_tries the (1-based) index of the draw that produced
 * the last of them, out_log_q_sampled[j] = log Q(out_ids[j]) with Q(c) = -expm1(num_tries log1p(-P(c))) (fp64, stored as fp32).
 * Draw t of step `step` is a pure function of (seed, step, t): word t & 3 of Philox4x32-10(counter = (t >> 2, 0x50726a45, step lo,
 * step hi), key = (seed lo, seed hi)), u = (word + 0.5) 2^-32, class = the first c with u < thresholds[c].  thresholds: device fp64
 * [n_classes], T[c] = log(c + 2) / log(n_classes + 1), built on the host.  All outputs are device pointers.  workspace:
 * oea_log_uniform_workspace_bytes() bytes, zeroed once; the call leaves it zeroed.  The call waits for the stream (it reads a
 * status word back).  n_sampled < 1, n_sampled > n_classes, a null pointer: OEA_EINVAL before any launch; more than
 * 64 n_sampled draws needed: OEA_EUNSUPPORTED (the outputs are then undefined). */
size_t oea_log_uniform_workspace_bytes(int64_t n_classes, int64_t n_sampled);
int oea_log_uniform_sample(int64_t n_classes, int64_t n_sampled, uint64_t seed, uint64_t step, const double *thresholds,
                           int32_t *out_ids, int64_t *out_num_tries, float *out_log_q_sampled, void *workspace, void *stream);
/* oea_proje_step: forward pass, gradients and TF's dense Adam (oea_adam_dense, beta1 0.9, beta2 0.999, eps 1e-8) of one ProjE batch.
 * The eight variables with their Adam moments, in this order: ent_embeds [n_ent, ld], rel_embeds [n_rel, ld] (both seen through the
 * row normalisation), entity_w [n_ent, ld], entity_b [n_ent], input bn beta, mlp_w, mlp_bias, output bn beta [dim].
 * pos int32 [n_pos, 3]; sampled / log_q_sampled [n_sampled] and num_tries (device int64[1], for log Q of the labels) as
 * oea_log_uniform_sample wrote them.  phase: OEA_PHASE_GRAD leaves the eight gradients readable through oea_proje_grads (dense
 * fp32, rows the batch did not touch are zero; the four vectors have stride 128), OEA_PHASE_APPLY runs Adam step t on them.
 * workspace: oea_proje_workspace_floats(n_ent, n_rel, dim, ld, max_pos, max_sampled) floats, zeroed once, for n_pos <= max_pos and
 * n_sampled <= max_sampled.  loss_accum += the batch loss.  dim > 128: OEA_EUNSUPPORTED; ld % 4 != 0, n_sampled < 2, n_pos < 1, a
 * null pointer: OEA_EINVAL -- both before anything is launched.  ids are not checked on the device.  One GPU. */
typedef struct oea_proje_vars {
    float *p[8], *m[8], *v[8];
} oea_proje_vars;
size_t oea_proje_workspace_floats(int64_t n_ent, int64_t n_rel, int32_t dim, int32_t ld, int64_t max_pos, int64_t max_sampled);
int oea_proje_grads(void *workspace, int64_t n_ent, int64_t n_rel, int32_t dim, int32_t ld, int64_t max_pos, int64_t max_sampled,
                    void **grads);
int oea_proje_step(const oea_proje_vars *vars, int64_t n_ent, int64_t n_rel, int32_t dim, int32_t ld, const int32_t *pos, int64_t n_pos,
                   const int32_t *sampled, const float *log_q_sampled, int64_t n_sampled, const int64_t *num_tries, int64_t t, float lr,
                   void *workspace, int64_t max_pos, int64_t max_sampled, double *loss_accum, int32_t phase, void *stream);

/* ---- ConvE (models/neural/conve.py) --------------------------------------------------------------------------------------------
 * oea_conve_step: forward pass, gradients and TF's dense Adam of one ConvE batch (csrc/conve_step.hip): the head and the relation
 * row, normalised, stacked into a [2x, y] image (x y = dim, x = the largest divisor of dim below sqrt(dim) + 1), batch norm,
 * dropout, a 3 x 3 'same' convolution into filter_num channels, batch norm, relu, dropout, a dense relu layer back to dim, batch
 * norm, and ProjE's sampled softmax.  The three batch norms are the affine map v gamma / sqrt(1 + 1e-3) + beta (inference mode on
 * the initial moving statistics).  The fourteen variables with their Adam moments, in this order: ent_embeds [n_ent, ld],
 * rel_embeds [n_rel, ld], entity_w [n_ent, ld], entity_b [n_ent], gamma1, beta1 [y], kern [3, 3, 1, F] (tap-major: (di 3 + dj) F
 * + f), cbias, gamma2, beta2 [F], fcW [2 dim F, ld] (row f 2 dim + image position; the pad columns stay zero), fcb, gamma3, beta3
 * [dim].  pos / sampled / log_q_sampled / num_tries, phase, workspace, loss_accum and t as for oea_proje_step;
 * oea_conve_grads gives the fourteen dense fp32 gradients after OEA_PHASE_GRAD.
 * Dropout: element e of layer L (0: the 2 dim inputs of the convolution, 1: the 2 dim F inputs of the dense layer, in the order
 * of fcW's rows) of batch row b at step mask_step is kept iff lane e & 7 of Philox4x32-10(counter = (e >> 3, 0x436f6e00 | L, b,
 * mask_step mod 2^32), key = (seed lo, seed hi)) is below floor(keep_prob 65536); lane l is the low (l even) or high (l odd) 16
 * bits of word l >> 1.  A kept element is multiplied by 1 / keep_prob.  keep_prob == 1 draws nothing and masks nothing.  The mask
 * does not depend on the batch size or on any tiling.
 * dim > 128, filter_num > 64: OEA_EUNSUPPORTED; keep_prob outside (0, 1], filter_num < 1, ld % 4 != 0, n_sampled < 2, n_pos < 1
 * or > max_pos, a null pointer: OEA_EINVAL -- both before anything is launched.  ids are not checked on the device.  One GPU. */
typedef struct oea_conve_vars {
    float *p[14], *m[14], *v[14];
} oea_conve_vars;
typedef struct oea_conve_cfg {
    int32_t filter_num;
    float keep_prob;
    uint64_t seed;
} oea_conve_cfg;
size_t oea_conve_workspace_floats(int64_t n_ent, int64_t n_rel, int32_t dim, int32_t ld, int32_t filter_num, int64_t max_pos,
                                  int64_t max_sampled);
int oea_conve_grads(void *workspace, int64_t n_ent, int64_t n_rel, int32_t dim, int32_t ld, int32_t filter_num, int64_t max_pos,
                    int64_t max_sampled, void **grads);
int oea_conve_step(const oea_conve_vars *vars, const oea_conve_cfg *cfg, int64_t n_ent, int64_t n_rel, int32_t dim, int32_t ld,
                   const int32_t *pos, int64_t n_pos, const int32_t *sampled, const float *log_q_sampled, int64_t n_sampled,
                   const int64_t *num_tries, uint64_t mask_step, int64_t t, float lr, void *workspace, int64_t max_pos,
                   int64_t max_sampled, double *loss_accum, int32_t phase, void *stream);

/* ---- IPTransE (approaches/iptranse.py) -----------------------------------------------------------------------------------------
 * The path half of train_loss (_generate_path_loss, iptranse.py:173-177, scaled by args.path_parm at iptranse.py:179-181):
 *   path_parm * sum_p (1 / w_p) relu(|x + y - r|^2 + margin - |x + y - r'|^2),  x, y, r, r' rows of Rn = l2n(rel) (rel itself when
 *   rel_l2_norm == 0); paths int32 [n, 3] = (r_x, r_y, r), neg_rel int32 [n] = r', weight fp32 [n] = w (the kernel multiplies by
 *   1 / w in fp32, the reference's tf.cast(1 / weight)).
 * Scores come from the Gram matrix G = Rn Rn^T, the gradient w.r.t. the normalised rows is A Rn for an R x R coefficient matrix A
 * built with scalar atomics (ten per active pair): two oea_gemm_tn_f32 products instead of O(n dim) row atomics
 * (csrc/ptranse_step.hip).  The rows of A Rn that an active pair refers to are ADDED to the relation gradient scratch (copy 0) of
 * the step workspace and their touched flags set; oea_triple_step_phase(..., OEA_PHASE_APPLY) then runs the optimiser.  loss_accum
 * += the path loss (path_parm included).  path_workspace: oea_path_workspace_bytes(n_rel, ld) bytes, zero-initialised once; the
 * call leaves its zero part zeroed again.  n == 0 is legal and launches nothing.
 * n_rel > 2048: OEA_EUNSUPPORTED; ld % 4 != 0, null pointer: OEA_EINVAL -- before anything is launched.  A path id (or r') outside
 * [0, n_rel) is found on the device: *err_flag = 3 and the batch adds nothing (no loss, no gradient); while *err_flag != 0 every
 * later batch is left out too -- the caller reads and clears the flag, as with the sampler's err_flag. */
size_t oea_path_workspace_bytes(int64_t n_rel, int32_t ld);
int oea_path_grad(const float *rel, int64_t n_rel, int32_t dim, int32_t ld, const int32_t *paths, const int32_t *neg_rel,
                  const float *weight, int64_t n, float margin, float path_parm, int32_t rel_l2_norm, void *step_workspace,
                  int64_t n_ent, void *path_workspace, double *loss_accum, int32_t *err_flag, void *stream);
/* One session.run([train_loss, optimizer]) of launch_ptranse_training_1epo (iptranse.py:250-268): the GRAD phase of the margin
 * step on (pos i, neg i), oea_path_grad with cfg->margin and cfg->rel_l2_norm, then ONE apply phase on the summed gradient.
 * loss_accum += triple loss + path_parm * path loss.  cfg: score_kind OEA_SCORE_TRANSE, loss_kind OEA_LOSS_MARGIN; cfg->l1 != 0 or
 * an optimiser other than SGD / Adagrad: OEA_EUNSUPPORTED (the reference asserts L2 and Adagrad, iptranse.py:140-142); n_rel and ld
 * as for oea_path_grad.  n_paths == 0: the plain margin step (path_workspace and err_flag may then be NULL).  A path id outside the
 * table drops the path half of that step only: its triple half still applies (the flag tells the caller). */
int oea_ptranse_step(float *ent, float *ent_acc, int64_t n_ent, float *rel, float *rel_acc, int64_t n_rel, int32_t dim, int32_t ld,
                     const int32_t *pos, int64_t n_pos, const int32_t *neg, int64_t n_neg, const int32_t *paths,
                     const int32_t *neg_rel, const float *weight, int64_t n_paths, float path_parm, const oea_step_cfg *cfg,
                     void *step_workspace, void *path_workspace, double *loss_accum, int32_t *err_flag, void *stream);
/* The path batches of a whole epoch in one launch (generate_batch, iptranse.py:77-85, for every step): P = (n1 + n2) / steps paths
 * per step, the first num1 = (int)((double)n1 / (n1 + n2) * P) from KG1's list (paths1 int32 [n1, 3], weight1 fp32 [n1]), the rest
 * from KG2's.  random.sample(paths, num) = the first num images of a keyed permutation of the list (oea_perm_index, key from
 * Philox4x32-10(seed; epoch, step, side)): no repeats inside a step and side.  r' = a Philox-uniform element of the relation list of
 * the KG the path came from (generate_neg_paths, iptranse.py:21-26; it may equal r, the reference does not filter).
 * out_paths int32 [steps, P, 3], out_neg_rel int32 [steps, P], out_weight fp32 [steps, P].  Reads no table: it can run ahead on a
 * side stream.  P == 0 launches nothing. */
int oea_path_sample_epoch(const int32_t *paths1, const float *weight1, int64_t n1, const int32_t *paths2, const float *weight2,
                          int64_t n2, const int32_t *rels1, int32_t n_rels1, const int32_t *rels2, int32_t n_rels2, int32_t steps,
                          uint64_t seed, uint32_t epoch, int32_t *out_paths, int32_t *out_neg_rel, float *out_weight, void *stream);
/* `steps` x oea_ptranse_step enqueued by ONE call (launch_ptranse_training_1epo's loop, iptranse.py:252-268), no host read and no
 * allocation inside: batch s = rows [offsets_host[s], offsets_host[s + 1]) of pos_all and of neg_buf (the epoch's negatives already
 * drawn, one per positive: the layout oea_triple_epoch_range takes with side0 == side1 == NULL and k = 1) with the path batch s of
 * oea_path_sample_epoch's three buffers.  P == 0: plain margin steps. */
int oea_ptranse_epoch(float *ent, float *ent_acc, int64_t n_ent, float *rel, float *rel_acc, int64_t n_rel, int32_t dim, int32_t ld,
                      const int32_t *pos_all, const int64_t *offsets_host, int32_t steps, const int32_t *neg_buf,
                      const int32_t *path_buf, const int32_t *neg_rel_buf, const float *weight_buf, int64_t P, float path_parm,
                      const oea_step_cfg *cfg, void *step_workspace, void *path_workspace, double *loss_accum, int32_t *err_flag,
                      void *stream);
/* One session.run([alignment_loss, alignment_optimizer]) of launch_alignment_training_1epo (iptranse.py:288-301):
 * loss = sum_i weight[i] relu(|h + r - t|^2 + margin - |h' + r' - t'|^2) over the pairs (pos i, neg i), rows from the
 * (normalised) tables (_generate_transe_alignment_loss, iptranse.py:167-170); one wave per pair, the gradient rows into the step
 * scratch with the engine's own atomics, then the apply phase.  cfg: margin, ent_l2_norm / rel_l2_norm, opt_kind SGD or Adagrad, lr;
 * l1 != 0, Adam / Adadelta: OEA_EUNSUPPORTED.  loss_accum += the batch loss. */
int oea_weighted_pair_step(float *ent, float *ent_acc, int64_t n_ent, float *rel, float *rel_acc, int64_t n_rel, int32_t dim,
                           int32_t ld, const int32_t *pos, const int32_t *neg, const float *weight, int64_t n,
                           const oea_step_cfg *cfg, void *step_workspace, double *loss_accum, void *stream);

/* ---------------------------------------------------------------------------------------
 * Negative sampling -- replaces generate_neg_triples_fast (modules/train/batch.py:89-119).
 * The membership set replaces the python set `all_triples_set`.
 * ------------------------------------------------------------------------------------- */
/* capacity: power of two >= 2*n;  table: uint64[capacity] on the device */
uint64_t oea_tripleset_capacity(int64_t n);
int oea_tripleset_build(const int32_t *triples, int64_t n, uint64_t *table, uint64_t capacity,
                        void *stream);
/* out[p*k + s] = s-th negative of positive p.  candidates = nbr[ent_pos[e]*nbr_k ...] when
 * nbr != NULL (truncated sampling, neighbor.get(e), batch.py:96-97) else entity_list.
 * RNG stream: Philox4x32-10 keyed by seed, counter (p + pos_offset, step, try, draw). */
int oea_sample_negatives(const int32_t *pos, int64_t n_pos, int32_t k, const uint64_t *table,
                         uint64_t capacity, const int32_t *entity_list, int32_t n_ent_list,
                         const int32_t *ent_pos, const int32_t *nbr, int32_t nbr_k, uint64_t seed,
                         uint32_t step, uint32_t pos_offset, int32_t max_try, int32_t *out,
                         int32_t *err_flag, void *stream);

/* The same kernel fed from a RECORD of the reference's own draws instead of Philox (tests: pins the sampler's algorithm -- rounds,
 * one side per round, distinct draws, true triples removed except in the last round, order of acceptance -- against
 * generate_neg_triples_fast itself, modules/train/batch.py:89-119, which draws with python's Mersenne Twister and cannot be matched
 * draw by draw otherwise).  replay int32 [n_pos, max_try, 1 + k]: per positive and round, np.random.binomial's value (1 = corrupt
 * the head) followed by the POSITIONS in the candidate list of that round's random.sample (as many as were still needed; the rest
 * -1).  err_flag 2: a recorded position does not fit the candidate list. */
int oea_sample_negatives_replay(const int32_t *pos, int64_t n_pos, int32_t k, const uint64_t *table, uint64_t capacity,
                                const int32_t *entity_list, int32_t n_ent_list, const int32_t *ent_pos, const int32_t *nbr,
                                int32_t nbr_k, int32_t max_try, const int32_t *replay, int32_t *out, int32_t *err_flag, void *stream);

/* One launch for a whole (pos_batch1 + pos_batch2) batch of generate_relation_triple_batch
 * (batch.py:36-45): positives [0, n_split) are sampled against side[0] (KG1's triple set,
 * entity list and neighbours), positives [n_split, n_pos) against side[1] (KG2).  Identical
 * draws to two oea_sample_negatives calls with pos_offset and pos_offset + n_split. */
typedef struct oea_sampler_side {
    const uint64_t *table;
    uint64_t capacity;
    const int32_t *entity_list;
    const int32_t *ent_pos;
    const int32_t *nbr;      /* NULL: uniform sampling over entity_list */
    int32_t n_ent_list;
    int32_t nbr_k;
    const uint32_t *filter;  /* NULL, or oea_tripleset_filter_build's bit array over the same triples (round 6) */
    uint64_t filter_bits;
} oea_sampler_side;
/* A "certainly absent" pre-test for the membership probes of the sampler (batch.py:108-110: `set(neg_triples) - pos_triples`): one bit per
 * hash bucket, oea_tripleset_filter_bits(capacity) = 8 x capacity bits (1 MB for the 400,000 triples of a 100K KG: resident in every XCD's
 * L2, where the 8 MB key table is not).  A clear bit answers the probe; a set bit (all present triples, ~5 % of the absent ones) goes on to
 * the key table: the sampler's output is unchanged. */
uint64_t oea_tripleset_filter_bits(uint64_t capacity);
int oea_tripleset_filter_build(const int32_t *triples, int64_t n, uint32_t *filter, uint64_t filter_bits, void *stream);
int oea_sample_negatives_pair(const int32_t *pos, int64_t n_pos, int64_t n_split, int32_t k,
                              const oea_sampler_side *side0, const oea_sampler_side *side1, uint64_t seed,
                              uint32_t step, uint32_t pos_offset, int32_t max_try, int32_t *out,
                              int32_t *err_flag, void *stream);

/* Negatives of EVERY batch of an epoch in one launch: pos_all holds the batches back to back, batch s is
 * rows [offsets[s], offsets[s+1]) with its first splits[s] rows from KG1 (offsets_dev: int64 [steps+1],
 * splits_dev: int64 [steps], both on the DEVICE).  Draws are identical to `steps` calls of
 * oea_sample_negatives_pair with step = step_base + s (the sampler does not depend on the tables, so an
 * epoch's negatives can be drawn ahead of its optimiser steps). */
int oea_sample_negatives_epoch(const int32_t *pos_all, int64_t n_rows, const int64_t *offsets_dev,
                               const int64_t *splits_dev, int32_t steps, int32_t k, const oea_sampler_side *side0,
                               const oea_sampler_side *side1, uint64_t seed, uint32_t step_base, int32_t max_try,
                               int32_t *out_all, int32_t *err_flag, void *stream);

/* A whole epoch of BasicModel.launch_triple_training_1epo (basic_model.py:222-232) enqueued by
 * ONE call: for step in [0, steps): sample the negatives of batch `step`
 * (oea_sample_negatives_pair with Philox step = step_base + step) and run the fused optimiser
 * step.  oea_epoch describes the epoch -- what the plain, the partitioned and the boundary-row form of the call share.
 * pos_all holds the epoch's positive batches back to back; batch `step` is rows
 * [offsets_host[step], offsets_host[step+1]) of it and its first splits_host[step] rows belong
 * to KG1.  k == 0: positive-only losses (MTransE), no sampling.  When offsets_dev / splits_dev (device
 * copies of the two host arrays) are given, neg_buf must hold (total rows)*k triples and the whole
 * epoch is sampled by ONE launch up front (oea_sample_negatives_epoch); otherwise neg_buf holds
 * max_batch*k triples and every step samples its own batch.  side0 == side1 == NULL together with the device
 * layout: neg_buf ALREADY holds the epoch's negatives (drawn by the caller with oea_sample_negatives_epoch, typically
 * on a second stream while the previous epoch was still running).  Nothing is synchronised: the host returns after enqueueing ~3 kernels
 * per step, which removes the per-step host round trip of the reference's feed_dict loop. */
typedef struct oea_epoch {
    float *ent, *ent_acc;                /* entity table [n_ent, ld] and its optimiser state; under the entity-id partition */
    int64_t n_ent;                       /* (_comm / _halo) ent_acc is the state of the OWNED rows only: acc_own [rpr, ld] */
    float *rel, *rel_acc;
    int64_t n_rel;
    int32_t dim, ld;
    const int32_t *pos_all;              /* the batches */
    const int64_t *offsets_host, *splits_host;
    int32_t steps;
    const int64_t *offsets_dev, *splits_dev;
    int32_t k;                           /* sampling */
    const oea_sampler_side *side0, *side1;
    uint64_t seed;
    uint32_t step_base;                  /* Philox step of the epoch's step 0 */
    int32_t *neg_buf, *err_flag;
    const oea_step_cfg *cfg;
    void *workspace;
    double *loss_accum;
} oea_epoch;
/* Steps [step_begin, step_end) of the epoch (the whole epoch: 0, steps; a caller that stops or resumes inside an epoch -- e.g.
 * a benchmark timing K steps -- still enqueues them with one call).  A range with step_begin == 0 draws the whole epoch's
 * negatives into neg_buf in one launch when the device layout is given; a later range of the same epoch either passes
 * side0 == side1 == NULL (neg_buf still holds them) or both sides (its steps are then drawn again batch by batch -- identical
 * draws).
 *   rank, world  (0, 1: the whole batches)  ONE RANK of a job whose ranks take contiguous shares of every batch (rows
 *                [n rank / world, n (rank + 1) / world) of the batch's n rows, as models/dist.py:shard_batch) and train on LOCAL
 *                copies of the tables between two exchanges (`dp_exchange = 'epoch'`: no collective inside the epoch; the caller
 *                reconciles the copies at the epoch's end).  The negatives keep the single-process Philox streams (position inside
 *                the batch), so the union of the ranks' draws is the single-process draw.
 *   plan         (NULL: none; world == 1 only) the workspace of the epoch's gathered-sum plan, see below */
int oea_triple_epoch_range(const oea_epoch *e, int32_t step_begin, int32_t step_end, int32_t rank, int32_t world, void *plan,
                           size_t plan_bytes, int32_t plan_built, void *stream);

/* An epoch's shuffle and batch layout in one call (basic_model.py:234-235: random.shuffle of both KGs' relation-triple lists;
 * modules/train/batch.py:17-22: batch s = KG1's slice s then KG2's slice s): triples int32 [n1 + n2, 3] = list 1 then list 2 (never
 * modified), slot int64 [n_slots] = the fixed map "position in the epoch's batch layout -> position in cat(list1, list2)"; a fresh
 * uniform permutation of each list (Philox4x32-10 keys of (index, epoch) under `seed`, one stable radix sort) is applied under the
 * map: dall[j] = triples[perm[slot[j]]].  No allocation, no host read (side stream). */
size_t oea_epoch_layout_bytes(int64_t n);
int oea_epoch_layout(const int32_t *triples, int64_t n1, int64_t n2, const int64_t *slot, int64_t n_slots, uint64_t seed, uint32_t epoch,
                     int32_t *dall, void *workspace, size_t ws_bytes, void *stream);

/* ---- the gathered-sum plan of an epoch (round 6; csrc/step_plan.h) ------------------------------------------------------------
 * Replaces, for the rows of the positives' own heads and tails, the scatter-add TF performs on the gradient of
 * tf.nn.embedding_lookup (IndexedSlices -> unsorted_segment_sum, models/basic_model.py:89-98, modules/base/optimizers.py:4-7) --
 * which the step kernels otherwise do with fp32 atomics that execute memory-side on gfx950 (~20 G requests/s: 24 of 54 us of the
 * scoring kernel at the EN-FR-100K shape).  The epoch's positives and the negatives drawn ahead for them say BEFORE the epoch runs
 * which entity row receives which positive's gradient rows: oea_step_plan_build sorts those references by (step, row) once per
 * epoch (stable: batch order inside a row).  With a plan, the scoring kernel writes two rows per positive with plain stores and the
 * optimiser kernel (apply_rows_plan) gathers every listed row's sum in the plan's order -- deterministic for those rows -- and
 * visits exactly the rows that received gradient; relation rows, the corrupted rows of ACTIVE negatives and positives outside the
 * rule (negatives on mixed sides, entries that are no corruption of their positive) keep the atomic scratch and the flag-driven
 * optimiser pass.  Result = oea_triple_epoch_range up to the order of fp32 additions.
 *   oea_step_plan_supported  1 when an epoch under `cfg` would use a plan (TransE score, limited loss, both tables normalised,
 *                            1 <= k <= 10 == cfg->neg_group_k, ld <= 256, SGD / Adagrad, fp32 scratch, tables + state larger than
 *                            128 MB -- cache-resident tables keep the flag-driven optimiser pass, which is faster there --,
 *                            OEA_STEP_PLAN != 0; OEA_STEP_PLAN=2 drops the size condition)
 *   oea_step_plan_bytes      workspace of a plan for n_total positives in `steps` batches of at most max_batch rows (includes the
 *                            2 * max_batch contribution rows)
 *   oea_step_plan_build      pos_all [n_total, 3] in batch order, neg_all [n_total * k, 3] (oea_sample_negatives_epoch), offsets_dev
 *                            [steps + 1] int64 on the device; a few launches + four device primitives on `stream`, no allocation,
 *                            no host read: meant for a side stream behind the previous epoch.  Also leaves rel_order: every
 *                            step's positives (index inside the batch) in stable ascending order of relation id.  The planned
 *                            scoring kernel takes its positives in that order, so that a workgroup's 8 waves nearly always
 *                            share one relation and sum their relation rows on chip before ONE row of atomics
 *                            (OEA_STEP_REL_ORDER=0: batch order, one row of atomics per positive)
 *   oea_triple_epoch_range   takes the plan workspace as `plan`; plan_built = 0: the call builds the plan itself (on `stream`,
 *                            after drawing the negatives when it draws them); plan == NULL, world > 1 or an unsupported
 *                            configuration: the epoch without a plan. */
int32_t oea_step_plan_supported(const oea_step_cfg *cfg, int64_t n_ent, int64_t n_rel, int32_t ld, int32_t k);
size_t oea_step_plan_bytes(int64_t n_total, int32_t steps, int64_t max_batch, int64_t n_ent, int32_t ld);
int oea_step_plan_build(const int32_t *pos_all, const int32_t *neg_all, int32_t k, const int64_t *offsets_dev, int64_t n_total,
                        int32_t steps, int64_t max_batch, int64_t n_ent, int32_t ld, void *plan, size_t plan_bytes, void *stream);
/* byte offsets inside a plan workspace (for tests that hold a built plan to the oracle's restatement): out[0] sorted entry values
 * (uint32: sign << 31 | slot), [1] distinct keys (uint64: step << row_bits | row), [2] first entry of every distinct key (uint32),
 * [3] number of distinct keys (int32), [4] first distinct key of every step (int32 [steps + 1]), [5] contribution rows, [6] row_bits,
 * [7] total bytes, [8] per-positive hub bits (uint32 [n_total]: bit 0 / 1 = the positive's head / tail row has more than 8
 * references in its step and takes this positive's gradient through the atomic scratch instead); out has 9 elements */
int oea_step_plan_offsets(int64_t n_total, int32_t steps, int64_t max_batch, int64_t n_ent, int32_t ld, int64_t *out);
/* *out = byte offset of rel_order (uint32 [n_total]; for step s, rel_order[offsets[s] + i] = index inside the batch of the step's
 * i-th positive in stable ascending order of relation id = numpy.argsort(relations of the batch, kind="stable")) */
int oea_step_plan_rel_order_offset(int64_t n_total, int32_t steps, int64_t max_batch, int64_t n_ent, int32_t ld, int64_t *out);

/* The steps [step_begin, step_end) of a data-parallel epoch under the partition from ONE call, over the C ABI's own
 * communicator (oea_comm_*, declared below): per step GRAD on this rank's share of the batch (rows nb*rank/world ..
 * nb*(rank+1)/world of batch s, as oea_triple_epoch_range's rank / world) -> oea_part_pack -> reduce-scatter + relation all-reduce ->
 * oea_part_apply (+ oea_step_apply_normals for TransH) -> all-gather -> oea_part_unpack, all enqueued on `stream` with no host
 * work in between.  Buffers as above: send [world * rpr * (ld + 1)], own [rpr * (ld + 1)], rel_x [n_rel * (ld + 1)], upd
 * [rpr, ld], all [world, rpr, ld]; e->ent_acc = acc_own [rpr, ld] (Adagrad). */
struct oea_comm;
int oea_triple_epoch_range_comm(struct oea_comm *comm, const oea_epoch *e, int32_t step_begin, int32_t step_end, void *send, void *own,
                                void *rel_x, float *upd, float *all, void *stream);


/* Negative LINKS of AliNet.generate_input_batch (approaches/alinet.py:988-1006), drawn on the device.
 *   uniform   (nbr1 == NULL): pair q = round * n_pos + i, round < k:  (ents1[pi1_round(i)], ents2[pi2_round(i)])
 *             -- zip(random.sample(ents1, n_pos), random.sample(ents2, n_pos)) per round; needs n_pos <= n1, n2;
 *   truncated (nbr1 != NULL): pair q = link * 2k + slot:  slot < k: (e1, nbr1[row1[e1]][pi(slot)]),
 *             else (nbr2[row2[e2]][pi'(slot - k)], e2) -- random.sample(neighbors[e], k); needs k <= nbr_k;
 *             nbr1/nbr2: int32 [rows, nbr_k] neighbour entity ids, row1/row2: entity id -> row.
 * pi = keyed pseudo-random permutation (oea_perm_index; key from Philox4x32-10(seed; round | link, step)), i.e. draws
 * without replacement.  out_pairs int32 [m, 2] holds every draw, out_valid fp32 [m] is 1 for the pairs of
 * set(pairs) - exclude (first of equal pairs; exclude = oea_tripleset_build over (e1, 0, e2) triples, or NULL), 0 for
 * the rest.  m = k * n_pos (uniform) or 2 * k * n_pos.  scratch_keys / scratch_vals: uint64 / int32 [scratch_cap],
 * scratch_cap a power of two >= 2 m.  Errors mirror random.sample ("Sample larger than population"). */
uint32_t oea_perm_index(uint32_t i, uint32_t n, uint32_t key);
int oea_sample_link_negatives(const int32_t *pos_links, int64_t n_pos, int32_t k, const int32_t *ents1, int32_t n1,
                              const int32_t *ents2, int32_t n2, const int32_t *nbr1, const int32_t *row1,
                              const int32_t *nbr2, const int32_t *row2, int32_t nbr_k, const uint64_t *exclude,
                              uint64_t exclude_cap, uint64_t seed, uint32_t step, int32_t *out_pairs, float *out_valid,
                              uint64_t *scratch_keys, int32_t *scratch_vals, uint64_t scratch_cap, void *stream);

/* HOST arrays (the only entry point that takes host pointers besides oea_store_load/save_host): one-to-one
 * selection among candidate pairs by descending weight (ties: smaller left, then smaller right id), standing in for
 * the heuristic matching of modules/bootstrapping/alignment_finder.py:83-112.  selected[e] = 1 for the kept edges. */
int oea_greedy_matching(const int32_t *left, const int32_t *right, const float *weight, int64_t n_edges,
                        uint8_t *selected);
/* out[i] = <e1[ii[i]], e2[jj[i]]> over the first dim columns (device arrays): similarities of listed pairs
 * (sim_mat[x, y] lookups of the bootstrapping code). */
int oea_pair_dots(const float *e1, int32_t ld1, const float *e2, int32_t ld2, int32_t dim, const int32_t *ii,
                  const int32_t *jj, int64_t n, float *out, void *stream);

/* The k best (largest != 0: largest values; else smallest) of every row of a SHORT candidate matrix vals [n_rows, ld] (first nc <= 1,024
 * columns) by ranking, ties to the earlier column: out_sel int32 [n_rows, k] = the selected columns in ascending column order,
 * mapped through ids [n_rows, ld_ids] when given (NULL: the columns themselves); out_kth [n_rows] = the k-th best value.  Either
 * output may be NULL.  NaN sorts last in both directions (ties among NaNs by column, numpy's order; +-inf are ordinary values), so
 * every row writes exactly k slots.  What np.argsort / np.partition do on the [t, k + margin] candidate lists of RDGCN's get_neg
 * (approaches/rdgcn.py:75-87) and of calculate_nearest_k (modules/finding/similarity.py:80-83) after the grid prefilter. */
int oea_row_rank_select_f32(const float *vals, int64_t n_rows, int32_t nc, int64_t ld, int32_t k, int32_t largest, const int32_t *ids,
                            int64_t ld_ids, int32_t *out_sel, float *out_kth, void *stream);
int oea_row_rank_select_f64(const double *vals, int64_t n_rows, int32_t nc, int64_t ld, int32_t k, int32_t largest, const int32_t *ids,
                            int64_t ld_ids, int32_t *out_sel, double *out_kth, void *stream);

/* ---------------------------------------------------------------------------------------
 * Neighbour search -- replaces find_neighbours (modules/train/batch.py:157-165):
 * np.matmul(sub_embed, embed.T) + per-row np.argpartition(-row, k)[:k].
 * out_idx [nq, k]: the k columns with the largest inner product per query, selected by
 * (value desc, column asc), listed in ascending column order.  If id_map != NULL the
 * output holds id_map[col] (entity_list[neighbors_index], batch.py:163).
 * workspace: oea_topk_workspace_bytes(nq, nc) bytes (may be smaller: the call processes
 * query rows in chunks that fit `ws_bytes`; minimum one 128-row strip).
 * ------------------------------------------------------------------------------------- */
size_t oea_topk_workspace_bytes(int64_t nq, int64_t nc);
/* queries == candidates (q == c, the truncated-sampling refresh of one KG's entities against themselves): with a
 * workspace of this many bytes (0: shape not covered) oea_topk_inner computes only the tiles on and above the diagonal of
 * S = E E^T and feeds rows and columns from them (bit-identical result: S_ij == S_ji in the k-ordered fmaf chain).
 * That sweep multiplies the bf16 hi / lo split of the rows (approximate survivors, the neighbourhood of the k-th value
 * decided by exact chains: the same neighbour sets) and collects the survivors in per-wave record streams that a second kernel
 * deals to per-row lists.  Covered: 12,288 (OEA_TOPK_SYM_MIN) <= n <= 131,072 rows (1,024 tiles of 128), k / n up to a few
 * per cent.  Where the answer is 0 -- also under OEA_TOPK_BF16=0 (read once per process), and for 131,073..143,232 rows, which
 * per-row segment lists served until they were retired -- oea_topk_inner computes the full N x N sweep on the general list
 * path (nc >= 32,768) or the strips: the same neighbour sets; speed in that band not measured on either path. */
size_t oea_topk_sym_workspace_bytes(int64_t n, int32_t k);
int oea_topk_inner(const float *q, int64_t nq, int32_t ldq, const float *c, int64_t nc, int32_t ldc,
                   int32_t dim, int32_t k, const int32_t *id_map, int32_t *out_idx, void *workspace,
                   size_t ws_bytes, void *stream);

/* The selection half alone, on a similarity strip that already exists: out_idx[i, :] = the k columns
 * with the largest s[i, :] ((value desc, column asc), ascending column order).  RDGCN's hard-negative
 * mining (approaches/rdgcn.py:75-87: cdist cityblock + argsort()[0:k]) = oea_sim_matrix(manhattan)
 * + this call.  s 16-byte aligned, ld % 4 == 0 (rows are read 16 bytes at a time; the pad columns
 * nc..ld-1 are never selected whatever they hold). */
int oea_topk_rows(const float *s, int64_t n_rows, int64_t nc, int64_t ld, int32_t k, const int32_t *id_map,
                  int32_t *out_idx, void *stream);

/* ---------------------------------------------------------------------------------------
 * Alignment evaluation -- replaces sim() + calculate_rank() of greedy_alignment
 * (modules/finding/similarity.py:11-83, modules/finding/alignment.py:13-84,146-168).
 * Gold of row i is column gold_offset + i (gold_offset = 0 in the reference; a rank that owns
 * query rows [lo, hi) of a row-sharded evaluation passes gold_offset = lo and its csls_r slice).
 *   rank[i]   = #{j != i : S_ij > S_ii  or (S_ij == S_ii and j < i)}     (0-based)
 *   argmax[i] = smallest j maximising S_ij                               (rank[0])
 * metric: OEA_METRIC_*; csls_r / csls_c: per-row / per-column top-k means (NULL = no CSLS),
 * S'_ij = (2*S_ij - r_i) - c_j (similarity.py:74-76).
 * rank / argmax: int32 [n1].  workspace: oea_rank_workspace_bytes(n1) bytes.
 * Inner-product tiles (this call, oea_sim_matrix, oea_topk_inner): both operands are first copied into two
 * process-wide, grow-only scratch buffers in the packed layout the LDS-DMA staging reads ([n_pad, Kp], see
 * DESIGN.md "Packed similarity operands"); reuse is ordered by `stream` (a call on another stream waits for
 * the previous use).
 * ------------------------------------------------------------------------------------- */
enum { OEA_METRIC_INNER = 0, OEA_METRIC_MANHATTAN = 1, OEA_METRIC_EUCLIDEAN = 2,
       OEA_METRIC_MANHATTAN_F32 = 3 /* oea_sim_matrix only: 1 - sum |a - b| accumulated in fp32 -- a ranking pre-filter, not scipy's bits */ };
size_t oea_rank_workspace_bytes(int64_t n1);
int oea_rank_eval(const float *e1, int64_t n1, int32_t ld1, const float *e2, int64_t n2, int32_t ld2,
                  int32_t dim, int32_t metric, const float *csls_r, const float *csls_c, int64_t gold_offset,
                  int32_t *rank, int32_t *argmax, void *workspace, void *stream);
/* integer reductions of rank[]: hits[i] = #{rank < top_k[i]}, rank_sum = sum(rank+1) (int64),
 * rr_sum = sum 1/(rank+1) (double, fixed summation order).  alignment.py:163-168. */
/* Inner-product evaluation through a CERTIFIED bf16 prefilter (round 4): the tile sweep multiplies bf16 splits of the operands
 * (x = hi + lo: hi.hi + hi.lo + lo.hi on v_mfma_f32_32x32x16_bf16, 3/16 of the fp32 matrix time), counts the candidates that are
 * greater than the gold value beyond the error bound, and RECORDS the (query, candidate) pairs inside the bound of the gold value or
 * of the row's running maximum; a second kernel decides the records with the exact k-ordered fmaf chain.  rank / argmax are
 * those of oea_rank_eval(OEA_METRIC_INNER) bit for bit.  status int32[2] (device): [0] != 0 = the record buffer overflowed,
 * the results are INVALID and the caller must take oea_rank_eval; [1] = records written.  Workspace:
 * oea_rank_eval_bf16_workspace_bytes(n1, dim).  No CSLS terms here (oea_rank_eval_metrics_bf16 takes them). */
size_t oea_rank_eval_bf16_workspace_bytes(int64_t n1, int32_t dim);
int oea_rank_eval_bf16(const float *e1, int64_t n1, int32_t ld1, const float *e2, int64_t n2, int32_t ld2, int32_t dim,
                       int64_t gold_offset, int32_t *rank, int32_t *argmax, int32_t *status, void *workspace, void *stream);
/* oea_rank_eval_bf16 with the CSLS means (csls_r [n1] of the query rows, csls_c [n2]; both NULL = oea_rank_eval_bf16): what a rank
 * of a row-sharded evaluation calls for its block of query rows (gold_offset = its first row). */
int oea_rank_eval_bf16_csls(const float *e1, int64_t n1, int32_t ld1, const float *e2, int64_t n2, int32_t ld2, int32_t dim,
                            const float *csls_r, const float *csls_c, int64_t gold_offset, int32_t *rank, int32_t *argmax,
                            int32_t *status, void *workspace, void *stream);
/* the same + argmax + the metrics of oea_rank_metrics in one go: out int64 [nk + 4] (device) = hits[nk], sum(rank + 1), the bits of
 * the double sum 1 / (rank + 1) (the reduction order of oea_rank_metrics), overflow flag (!= 0: INVALID, take
 * oea_rank_eval_metrics), records written -- one device-to-host copy brings results and status back.  csls_r / csls_c (both or
 * neither): the CSLS means; the values ranked are then (2 s - csls_r[i]) - csls_c[j] as in oea_rank_eval. */
int oea_rank_eval_metrics_bf16(const float *e1, int64_t n1, int32_t ld1, const float *e2, int64_t n2, int32_t ld2, int32_t dim,
                               const float *csls_r, const float *csls_c, int64_t gold_offset, const int32_t *top_k_host, int32_t nk,
                               int32_t *rank, int32_t *argmax, int64_t *out_dev, void *workspace, void *stream);
/* the prefilter's approximate similarities out[i, j] ~ <e1[i], e2[j]> (tests of the error bound, timing) */
int oea_sim_bf16_matrix(const float *e1, int64_t n1, int32_t ld1, const float *e2, int64_t n2, int32_t ld2, int32_t dim, float *out,
                        int64_t ld_out, void *stream);
/* The inner-product evaluation in TWO launches (the 10,500^2 call spent a third of its time in eight small
 * launches around the 0.20 ms sweep): a prologue that packs both operands, computes the gold similarities and clears the
 * merge buffers, and the tile sweep, whose last workgroup extracts argmax and reduces the metrics in a fixed order.
 * hits_and_rank_sum_dev: int64 [nk + 1] (Hits@top_k[i] counts, then sum(rank + 1)); rr_sum_dev: double sum 1 / (rank + 1).
 * workspace: oea_rank_eval_metrics_workspace_bytes(n1).  Same ranks / argmax as oea_rank_eval + oea_rank_metrics. */
size_t oea_rank_eval_metrics_workspace_bytes(int64_t n1);
int oea_rank_eval_metrics(const float *e1, int64_t n1, int32_t ld1, const float *e2, int64_t n2, int32_t ld2, int32_t dim,
                          const float *csls_r, const float *csls_c, int64_t gold_offset, const int32_t *top_k_host, int32_t nk,
                          int32_t *rank, int32_t *argmax, int64_t *hits_and_rank_sum_dev, double *rr_sum_dev, void *workspace,
                          void *stream);
int oea_rank_metrics(const int32_t *rank, int64_t n, const int32_t *top_k_host, int32_t nk,
                     int64_t *hits_dev, int64_t *rank_sum_dev, double *rr_sum_dev, void *stream);

/* calculate_rank (alignment.py:146-168) on an explicit block of a similarity matrix s [n_rows, ld]
 * (device): gold of row i is column gold_idx[i] (0 <= gold_idx[i] < nc).  rank[i] = position of the
 * gold in the descending order of row i with the tie rule above, argmax[i] = smallest column of the
 * row maximum. */
int oea_rank_rows(const float *s, int64_t n_rows, int64_t nc, int64_t ld, const int32_t *gold_idx,
                  int32_t *rank, int32_t *argmax, void *stream);

/* Similarity strip S[i, j] for i in [0,n1), j in [0,n2): out is [n1, ld_out] fp32
 * (similarity.py:34-48).  Used by the sim() mirror, CSLS and the neighbour search. */
int oea_sim_matrix(const float *e1, int64_t n1, int32_t ld1, const float *e2, int64_t n2,
                   int32_t ld2, int32_t dim, int32_t metric, float *out, int64_t ld_out,
                   void *stream);
/* Fixed-point L1 pre-filter (RDGCN's hard-negative mining, approaches/rdgcn.py:75-87; scipy cdist 'cityblock' in the reference).
 * oea_quantize_rows_u16: dst[i, k] = clamp(round((src[i, k] - lo) * inv_step), 0, 65535) for k < dim, 0 for dim <= k < ldq
 * (ldq: a multiple of 8).  oea_l1_u16_strip: out[i, j] = -(float) sum_k |q[i, k] - c[j, k]| (integer sums; larger = nearer, the
 * order oea_topk_rows selects; sums >= 2^24 are rounded to float).  step * sum is within dim * step of the true L1 distance when
 * [lo, lo + 65535 step] covers the table: the caller certifies its candidate lists with that bound and re-ranks them with
 * oea_pair_l1_f64. */
int oea_quantize_rows_u16(const float *src, int64_t n, int32_t ld, int32_t dim, float lo, float inv_step, uint16_t *dst,
                          int32_t ldq, void *stream);
int oea_l1_u16_strip(const uint16_t *q, int64_t nq, const uint16_t *c, int64_t nc, int32_t ldq, float *out, int64_t ld_out,
                     void *stream);
/* Manhattan evaluation of a block of query rows from their grid distances (strip [rows, ld] = oea_l1_u16_strip of rows
 * row0 .. row0 + rows of e1 against all nc rows of e2; step = the grid's step, err = the bound on |distance - G step|):
 * rank[row0 + r] / argmax[row0 + r] as oea_rank_eval(OEA_METRIC_MANHATTAN) gives them -- candidates whose grid distance
 * leaves no doubt are counted from the strip, the others by their exact similarity (sequential fp64 chain).
 * gold of row i = column gold_offset + i.  n_exact_rows (may be NULL): incremented for every row whose candidate lists
 * overflowed and which therefore evaluated every pair exactly inside the kernel -- many of them mean the table's range makes
 * the grid's error bound useless and the all-pairs kernel (oea_rank_eval) is the faster path. */
int oea_rank_l1_grid_rows(const float *strip, int64_t rows, int64_t row0, int64_t nc, int64_t ld, const float *e1, int32_t ld1,
                          const float *e2, int32_t ld2, int32_t dim, int64_t gold_offset, float step, float err, int32_t *rank,
                          int32_t *argmax, int32_t *n_exact_rows, void *stream);
/* The same with CSLS (models/basic_model.py:132-135: test() evaluates a second time with csls = args.csls; GCN-Align and RDGCN
 * do so under the manhattan metric): rank / argmax of v_ij = (2 s_ij - csls_r[i]) - csls_c[j] as oea_rank_eval gives them with
 * the same means.  csls_r [n1], csls_c [nc]. */
int oea_rank_l1_grid_rows_csls(const float *strip, int64_t rows, int64_t row0, int64_t nc, int64_t ld, const float *e1, int32_t ld1,
                               const float *e2, int32_t ld2, int32_t dim, int64_t gold_offset, float step, float err,
                               const float *csls_r, const float *csls_c, int32_t *rank, int32_t *argmax, int32_t *n_exact_rows,
                               void *stream);
/* exact manhattan SIMILARITIES of a candidate list: out[i, j] = float(1 - sum_k |q[i, k] - table[cand[i, j], k]|) with the
 * sequential fp64 chain of oea_sim_matrix(OEA_METRIC_MANHATTAN) (k ascending: scipy cdist's bits) -- the values the CSLS means
 * of the manhattan metric are sums of (modules/finding/similarity.py:46-48,57-83). */
int oea_pair_l1_sim(const float *q, int64_t nq, int32_t ldq, const float *table, int64_t n, int32_t ldt, int32_t dim,
                    const int32_t *cand, int32_t c, float *out, void *stream);
/* exact fp64 L1 distances of a candidate list: out[i, j] = sum_k |q[i, k] - table[cand[i, j], k]| (fixed summation order).
 * With OEA_METRIC_MANHATTAN_F32 + oea_topk_rows this is RDGCN's hard-negative mining (approaches/rdgcn.py:75-87) without the
 * fp64 distance of every (seed, entity) pair: fp32 ranks k + margin candidates, these are re-ranked exactly. */
int oea_pair_l1_f64(const float *q, int64_t nq, int32_t ldq, const float *table, int64_t n, int32_t ldt, int32_t dim,
                    const int32_t *cand, int32_t c, double *out, void *stream);

/* out[i] = mean of the k largest of S[i, 0:n2] (calculate_nearest_k, similarity.py:80-83),
 * summed in descending order in fp32.  k <= 64. */
int oea_row_topk_mean(const float *s, int64_t n1, int64_t n2, int64_t ld, int32_t k, float *out,
                      void *stream);
/* CSLS means in one sweep (calculate_nearest_k of S and of S^T, similarity.py:60-65,80-83) for the inner-product metric,
 * without S in HBM: r_out[i] = mean of the k largest of row i of e1 e2^T, c_out[j] = the same for column j -- equal to
 * oea_row_topk_mean on the strips of S and S^T bit for bit.  n1, n2 >= 4096 and k <= 32 (otherwise OEA_EUNSUPPORTED and
 * the caller takes the strip route); workspace: oea_csls_means_workspace_bytes (0 = shape not covered). */
size_t oea_csls_means_workspace_bytes(int64_t n1, int64_t n2, int32_t k);
int oea_csls_means(const float *e1, int64_t n1, int32_t ld1, const float *e2, int64_t n2, int32_t ld2, int32_t dim, int32_t k,
                   float *r_out, float *c_out, void *workspace, size_t ws_bytes, void *stream);
/* in place S'_ij = (2*S_ij - r_i) - c_j (csls_sim, similarity.py:74-76) */
int oea_csls_apply(float *s, int64_t n1, int64_t n2, int64_t ld, const float *r, const float *c,
                   void *stream);

/* ---------------------------------------------------------------------------------------
 * Neighbour aggregation -- replaces tf.sparse_tensor_dense_matmul(A, X)
 * (approaches/gcn_align.py:83,259; alinet.py:581; rdgcn.py:187,196) and its gradient.
 * CSR: rowptr int32 [n_rows+1], colidx int32 [nnz], vals fp32 [nnz].
 *   y[i, :] = act( sum_e vals[e] * x[colidx[e], :] )      act: 0 none, 1 relu
 * The backward pass is the same call on the transposed CSR.  mask_from (may be NULL):
 * y = y * (mask_from > 0) -- the relu gradient gate fused into the backward aggregate.
 * ------------------------------------------------------------------------------------- */
/* Optional work split for hub rows (degrees are power-law; ids are frequency-ordered, read.py:64-79):
 * rows with more than `threshold` (>= 96) nonzeros are cut on the host into chunks that different
 * workgroups sum and add atomically; `rows` lists those rows (zeroed before, activation / mask applied
 * after).  NULL = no splitting (a hub row is then summed by one workgroup). */
typedef struct oea_csr_split {
    const int32_t *chunk_row;   /* [n_chunks] row of each chunk */
    const int32_t *chunk_e0;    /* [n_chunks] first nonzero */
    const int32_t *chunk_e1;    /* [n_chunks] one past the last nonzero */
    const int32_t *rows;        /* [n_rows]   the split rows */
    int32_t n_chunks, n_rows, threshold;
    /* optional (NULL / 0: the chunks are added to y with atomics after a zeroing launch): with a buffer of
     * partials_floats >= n_chunks * ldy floats and the chunk range of every split row, the chunks are computed inside
     * the row kernel's launch and summed in chunk order by the epilogue -- two launches, deterministic */
    const int32_t *row_chunk0;  /* [n_rows + 1] first chunk of each split row */
    float *partials;
    int64_t partials_floats;
    /* optional, with `partials`: [n_rows] zero-initialised tickets -- the last chunk of a row to finish adds the row's
     * chunks in chunk order and stores the row inside the SAME launch (no epilogue launch; the tickets reset themselves) */
    uint32_t *tickets;
} oea_csr_split;
int oea_spmm_csr(const int32_t *rowptr, const int32_t *colidx, const float *vals, int64_t n_rows,
                 const float *x, int32_t dim, int32_t ldx, int32_t act, const float *mask_from,
                 float *y, int32_t ldy, const oea_csr_split *split, void *stream);

/* ---------------------------------------------------------------------------------------
 * Sparse graph attention -- replaces tf.nn.leaky_relu(values) -> tf.sparse_softmax ->
 * tf.sparse_tensor_dense_matmul and their gradients (approaches/alinet.py:661-676,
 * rdgcn.py:202-215).  Segment s owns edges [seg_ptr[s], seg_ptr[s+1]) (the entries normalised
 * together -- whole rows, or TF1's consecutive runs) and adds its aggregate to output
 * row seg_row[s].  z: per-edge pre-activation logits; v: [n_cols, ld] values.
 *   alpha_e = softmax_seg(leaky_relu(z_e)) ;  out[seg_row[s]] += sum_e alpha_e * v[colidx[e]]
 * Backward: dz[e] and dv [n_cols, ld] from dout.
 * ------------------------------------------------------------------------------------- */
typedef struct oea_attn_graph {
    /* segments are cut into sub-segments of bounded length on the host (power-law degrees: a hub
     * row must not become one wave's serial loop); sub-segments of a segment are consecutive */
    const int32_t *sub_ptr;      /* [n_sub+1] edge range of each sub-segment */
    const int32_t *sub_seg;      /* [n_sub]   segment a sub-segment belongs to */
    const int32_t *seg_sub_ptr;  /* [n_seg+1] sub-segment range of each segment */
    const int32_t *seg_row;      /* [n_seg]   output row of each segment */
    const int32_t *colidx;       /* [nnz]     value row (column) of each edge */
    int64_t n_sub, n_seg, nnz;   /* nnz = sub_ptr[n_sub]: the number of edges */
    /* the aggregate out = P . v as a CSR over the OUTPUT rows (fixed summation order: slot order inside a row) */
    const int32_t *agg_rowptr;   /* [agg_rows+1] slot range of each output row */
    const int32_t *agg_colidx;   /* [nnz] value row of each slot */
    const int32_t *agg_edge;     /* [nnz] edge id of each slot (index into alpha); NULL: slot == edge (canonical order) */
    int64_t agg_rows;
    const oea_csr_split *agg_split;   /* hub rows of the aggregate (relative to agg_row0), or NULL */
    /* the transposed CSR for dv = P^T . dout */
    const int32_t *t_rowptr;     /* [t_rows+1] incoming-slot range of each value row (column) */
    const int32_t *t_row;        /* [nnz] output row of the incoming edge (row of dout) */
    const int32_t *t_edge;       /* [nnz] its edge id (index into alpha) */
    int64_t t_rows;
    const oea_csr_split *t_split;     /* hub columns (relative to t_row0), or NULL */
    /* the ranges a call works on (whole graph: [0, n)); a rank of a row-sharded job passes the whole graph with ITS
     * ranges: a block of segments (sub-segment range [sub0, sub1) = segments [seg0, seg1)), a block of output rows
     * [agg_row0, agg_row1) with slots [agg_slot0, agg_slot1) = agg_rowptr[agg_row0 / agg_row1], a block of columns */
    int64_t sub0, sub1, seg0, seg1;
    int64_t agg_row0, agg_row1, agg_slot0, agg_slot1;
    int64_t t_row0, t_row1, t_slot0, t_slot1;
} oea_attn_graph;
#define OEA_ATTN_ALPHA 1       /* forward: softmax statistics + alpha[e] of the segments [seg0, seg1) */
#define OEA_ATTN_AGGREGATE 2   /* forward: out rows [agg_row0, agg_row1) from alpha of ALL their edges */
#define OEA_ATTN_DZ 1          /* backward: dz[e] of the segments [seg0, seg1) */
#define OEA_ATTN_DV 2          /* backward: dv rows [t_row0, t_row1) */
size_t oea_sparse_attn_workspace_floats(const oea_attn_graph *g);
/* No atomics: results are bit-reproducible.  z, alpha, dz are indexed by edge id; out [agg_rows, ld], dv [t_rows, ld]:
 * every row of the call's range is written (rows without edges get zeros).  `phases` selects what runs (a single
 * process passes both bits; between the phases a sharded job all-gathers alpha / dz). */
int oea_sparse_attn_fwd(const oea_attn_graph *g, const float *z, const float *v, int32_t dim, int32_t ld,
                        float lrelu_slope, float *out, float *alpha, float *workspace, int32_t phases, void *stream);
int oea_sparse_attn_bwd(const oea_attn_graph *g, const float *z, const float *v, const float *alpha,
                        const float *dout, int32_t dim, int32_t ld, float lrelu_slope, float *dz, float *dv,
                        float *workspace, int32_t phases, void *stream);
/* The softmax half of the backward alone, for groups whose values are attached to ANOTHER pattern than the one they were
 * normalised over (the third reading of alinet.py:670-676's tf.sparse_softmax on a non-canonical tensor, SURVEY H3: row softmax
 * of the canonically sorted values, p-th value re-attached to the p-th index as fed): dz holds d alpha per edge on entry (the
 * caller's oea_pair_dots over the as-fed pattern) and d z = alpha (d alpha - sum_group alpha d alpha) lrelu'(z) on exit, for
 * the sub-segments [sub0, sub1).  Same kernels and summation order as oea_sparse_attn_bwd's OEA_ATTN_DZ phase. */
int oea_sparse_attn_dz(const oea_attn_graph *g, const float *z, const float *alpha, float *dz, float lrelu_slope,
                       float *workspace, void *stream);

/* ---------------------------------------------------------------------------------------
 * Row-wise glue of the GNN approaches, fused (csrc/gnn_fused.hip): one pass forward, one pass backward, one wave per
 * row, no atomics.  All tensors fp32 row-major.
 *
 * oea_concat_l2n_*: emb = l2n(concat(l2n(x_0), ..., l2n(x_{k-1}))), k <= 4 blocks [n, lds[i]] with dims[i] columns
 *   (approaches/alinet.py:835-840 / 932-943); out [n, ld_out], ld_out >= sum dims (pad columns get zeros);
 *   inv_blk [n, 4] / inv_all [n]: the inverse norms, kept for the backward.  bwd: dz [n, ld_out] -> dx[i] [n, lds[i]].
 * oea_pair_loss_l2_*: alinet.py:828-850 (compute_loss).  pairs int32 [m, 2], the first n_pos of them positive links:
 *   term_p = ||e_i - e_j||^2 (positive) | balance * weight * relu(margin - ||e_i - e_j||^2) (negative; weight [m - n_pos]
 *   or NULL = 1); the loss is the sum of terms [m] (the caller adds them: fixed order); coef [m] = d term / d ||.||^2.
 *   bwd = oea_pair_grad_rows(norm = 2): rowptr [n + 1] / other [2 m] / slot_pair [2 m] = the pairs' endpoints grouped by
 *   embedding row (slot order = the summation order), gscale = device scalar d L / d loss (NULL = 1); grad [n, ld]: every
 *   row written.  norm = 1: grad[r] = sum coef sign(e_r - e_other) -- the L1 hinge of GCN-Align (oea_align_loss_l1_coef).
 * oea_highway_*: gate = relu(tanh(p)), out = tanh(b' (1 - gate) + a' gate), a' = a gamma + beta, b' = b gamma + beta
 *   (alinet.py:597-622; gamma / beta = the layer's BatchNormalization affine, gamma already divided by sqrt(1 + eps));
 *   bwd: da, db, dp [n, d] and partials [oea_colsum_blocks(n), 2, d] whose sums over dim 0 are d gamma, d beta.
 * oea_bias_tanh_*: y = tanh(x + bias) (alinet.py:583-590); bwd: gx [n, d], partials [oea_colsum_blocks(n), d] -> d bias.
 * ------------------------------------------------------------------------------------- */
int oea_concat_l2n_fwd(const float *const *x, const int32_t *dims, const int32_t *lds, int32_t k, int64_t n, float *out,
                       int32_t ld_out, float *inv_blk, float *inv_all, void *stream);
int oea_concat_l2n_bwd(float *const *dx, const int32_t *dims, const int32_t *lds, int32_t k, int64_t n, const float *z,
                       const float *dz, int32_t ld_out, const float *inv_blk, const float *inv_all, void *stream);
int oea_pair_loss_l2_fwd(const float *emb, int64_t n, int32_t dim, int32_t ld, const int32_t *pairs, int64_t m, int64_t n_pos,
                         const float *weight, float margin, float balance, float *coef, float *terms, void *stream);
int oea_pair_grad_rows(const float *emb, int64_t n, int32_t dim, int32_t ld, const int32_t *rowptr, const int32_t *other,
                       const int32_t *slot_pair, const float *coef, const float *gscale, int32_t norm, float *grad, void *stream);
/* out[s] = sum of vals[order[e]] (order NULL: vals[e]) over e in [seg_ptr[s], seg_ptr[s + 1]) -- one wave per segment, fixed
 * order: the gradient of a gather from few distinct rows (rdgcn.py:202-215: per-relation logits gathered per attention edge) */
int oea_segment_sum_f32(const float *vals, const int32_t *order, const int32_t *seg_ptr, int64_t n_seg, float *out, void *stream);
/* the row-grouped endpoint lists of a pair list for oea_pair_grad_rows: pairs int32 [m, 2] with rows in [0, n_rows) ->
 * rowptr [n_rows + 1], other [2 m] (the partner row of every slot), slot_pair [2 m] (its pair); inside a row the slots keep
 * pair order.  One call, stream-ordered, no host synchronisation (csrc/graph_build.hip: rocPRIM stable sort + scan). */
int oea_pair_rows_build(const int32_t *pairs, int64_t m, int64_t n_rows, int32_t *rowptr, int32_t *other, int32_t *slot_pair,
                        void *stream);
int32_t oea_colsum_blocks(int64_t n);
int oea_highway_fwd(const float *a, const float *b, const float *p, const float *gamma, const float *beta, int64_t n, int32_t d,
                    float *out, void *stream);
int oea_highway_bwd(const float *a, const float *b, const float *p, const float *gamma, const float *beta, const float *out,
                    const float *gout, int64_t n, int32_t d, float *da, float *db, float *dp, float *partials, void *stream);
/* out [k1, ld_out] = A^T B for row-major A [m, lda] (k1 columns used) and B [m, ldb] (k2 columns): the weight gradient
 * dW = X^T dY of the GNN approaches' dense layers (alinet.py:574-582, rdgcn.py:250-256: m = #entities, k <= 500) on
 * v_mfma_f32_32x32x2_f32 (exact fp32 products, fixed summation order: slab order inside a row chunk, then chunk order).
 * k1, k2, lda, ldb multiples of 4, operands 16-byte aligned.  workspace: oea_gemm_tn_workspace_floats(m, k1, k2) floats
 * (partial tiles of the row chunks; 0 when one chunk suffices). */
size_t oea_gemm_tn_workspace_floats(int64_t m, int32_t k1, int32_t k2);
int oea_gemm_tn_f32(const float *a, int32_t lda, int32_t k1, const float *b, int32_t ldb, int32_t k2, int64_t m, float *out,
                    int32_t ld_out, float *workspace, void *stream);
/* The same product cut at its row chunks for a row-sharded job (the weight gradients dW = X^T dY of the GNN approaches' dense
 * layers, approaches/alinet.py:574-582): oea_gemm_tn_plan gives the chunk count and rows per chunk of the single-process call;
 * a rank runs oea_gemm_tn_partial on ITS chunks (slots [chunk_begin, chunk_end) of workspace [chunks][k1 * k2]), the slots are
 * all-gathered, and oea_gemm_tn_reduce adds all of them in chunk order -- the single-process summation order: same bits. */
int oea_gemm_tn_plan(int64_t m, int32_t k1, int32_t k2, int32_t *chunks, int64_t *rows_per_chunk);
int oea_gemm_tn_partial(const float *a, int32_t lda, int32_t k1, const float *b, int32_t ldb, int32_t k2, int64_t m,
                        int32_t chunk_begin, int32_t chunk_end, float *workspace, void *stream);
int oea_gemm_tn_reduce(const float *workspace, int32_t chunks, int32_t k1, int32_t k2, float *out, int32_t ld_out, void *stream);

/* RDGCN's dense glue between its sparse operators, one pass each way (rdgcn.py:184-191, 250-256, 330-333):
 * oea_sigmoid_mix_*: gate = sigmoid(p + bias), out = gate b + (1 - gate) a (highway; p = a W from a library GEMM);
 *   bwd: da, db, dp [n, d] and partials [oea_colsum_blocks(n), d] -> d bias (summed in block order by the caller); b_relu != 0:
 *   b is a relu's output and db is gated by b > 0 (the gradient of the relu's input).
 * oea_relu_axpy_*: out = x + alpha relu(y); bwd: dy = alpha gout where y > 0 (dx = gout).
 * oea_colsum_prod: partials [oea_colsum_blocks(n), d] of the column sums of x * y (d w0 of the diagonal layer). */
int oea_sigmoid_mix_fwd(const float *a, const float *b, const float *p, const float *bias, int64_t n, int32_t d, float *out,
                        void *stream);
int oea_sigmoid_mix_bwd(const float *a, const float *b, const float *p, const float *bias, const float *gout, int64_t n, int32_t d,
                        int32_t b_relu, float *da, float *db, float *dp, float *partials, void *stream);
int oea_relu_axpy_fwd(const float *x, const float *y, float alpha, int64_t total, float *out, void *stream);
int oea_relu_axpy_bwd(const float *y, const float *gout, float alpha, int64_t total, float *dy, void *stream);
int oea_colsum_prod(const float *x, const float *y, int64_t n, int32_t d, float *partials, void *stream);
int oea_bias_tanh_fwd(const float *x, const float *bias, int64_t n, int32_t d, float *y, void *stream);
int oea_bias_tanh_bwd(const float *y, const float *gy, int64_t n, int32_t d, float *gx, float *partials, void *stream);

/* Dense Adam step with tf.train.AdamOptimizer semantics (alinet.py:871, rdgcn.py:332); t = 1-based
 * step count. */
int oea_adam_dense(float *param, const float *grad, float *m, float *v, int64_t n, float lr, float beta1,
                   float beta2, float eps, int64_t t, void *stream);

/* L1 alignment hinge of GCN-Align / RDGCN (approaches/gcn_align.py:298-320,
 * rdgcn.py:293-315): forward + gradient w.r.t. the output embedding table.
 * ILL int32 [t,2]; neg_*: int32 [t*k]; grad [n, ld] must be zero on entry.
 * loss_accum += (sum L1 + sum L2) / (2 k t). */
int oea_align_loss_l1(const float *out_emb, int64_t n, int32_t dim, int32_t ld, const int32_t *ill,
                      int64_t t, int32_t k, float gamma, const int32_t *neg_left,
                      const int32_t *neg_right, const int32_t *neg2_left, const int32_t *neg2_right,
                      float *grad, double *loss_accum, void *stream);

/* The same hinge WITHOUT the gradient: coef_out [t + 2 t k] gets the signed coefficient of every pair -- [0, t): the links,
 * + #active hinges / (2 k t); [t + a 2k + i]: negative i of link a (i < k: (neg_left, neg_right), else (neg2_left,
 * neg2_right)), - 1 / (2 k t) if its hinge is active, else 0 -- and oea_pair_grad_rows(norm = 1) over the pairs' endpoints
 * grouped by row gives the gradient without atomics (reproducible; the choice when the negatives stay for several epochs
 * and k is small: GCN-Align).  grad may be NULL then. */
int oea_align_loss_l1_coef(const float *out_emb, int64_t n, int32_t dim, int32_t ld, const int32_t *ill,
                           int64_t t, int32_t k, float gamma, const int32_t *neg_left,
                           const int32_t *neg_right, const int32_t *neg2_left, const int32_t *neg2_right,
                           float *grad, double *loss_accum, float *coef_out, void *stream);

/* W -= lr * dW where dW is the gradient w.r.t. T = l2_normalize(W) pulled back through the
 * normalisation (gcn_align.py:52-56 + GradientDescentOptimizer, gcn_align.py:511).
 * normalize == 0: plain SGD. */
int oea_sgd_rows(float *w, const float *grad_t, int64_t rows, int32_t dim, int32_t ld,
                 int32_t normalize, float lr, void *stream);

/* One full-batch epoch of a GCN_Align_Unit (approaches/gcn_align.py:498-539: GraphConvolution(relu, trunc_normal weight) ->
 * GraphConvolution(identity, no weight) + align_loss + GradientDescentOptimizer; the loop of :737-785) enqueued by ONE call:
 *   T = l2_normalize(W);  X = T (featureless) | F . T;  H1 = relu(A X);  out = A H1;  hinge -> d out;
 *   d H1 = A^T d out (gated by H1 > 0);  d X = A^T d H1;  d T = d X | F^T d X;  W -= lr * (d T through the normalisation).
 * A / A^T / F / F^T: CSR operands (+ optional hub-row splits); pair_*: the hinge's pair endpoints grouped by row
 * (oea_align_loss_l1_coef + oea_pair_grad_rows(norm 1): no atomics) or NULL (oea_align_loss_l1 with atomics).
 * Buffers [n, ld] (t: [w_rows, ld]; x, g_t only with features; coef [t + 2 t k] only with pair lists) are the caller's
 * and hold the forward / backward intermediates afterwards (out = the unit's output embedding). */
typedef struct oea_gcn_unit {
    const int32_t *a_rowptr, *a_colidx; const float *a_vals; const oea_csr_split *a_split;
    const int32_t *at_rowptr, *at_colidx; const float *at_vals; const oea_csr_split *at_split;
    const int32_t *f_rowptr, *f_colidx; const float *f_vals; const oea_csr_split *f_split;       /* NULL: featureless */
    const int32_t *ft_rowptr, *ft_colidx; const float *ft_vals; const oea_csr_split *ft_split;
    const int32_t *row_ids;          /* [w_rows] = 0 .. w_rows - 1 */
    const int32_t *ill;              /* [t, 2] seed links */
    const int32_t *neg_left, *neg_right, *neg2_left, *neg2_right;      /* [t k] */
    const int32_t *pair_rowptr, *pair_other, *pair_slot;               /* [n + 1], [2 (t + 2 t k)] x 2, or NULL */
    int64_t n, w_rows, t;
    int32_t dim, ld, k;
    float gamma, lr;
} oea_gcn_unit;
typedef struct oea_gcn_unit_buffers {
    float *t, *x, *h1, *out, *g_out, *g_pre1, *g_x, *g_t, *coef;
} oea_gcn_unit_buffers;
int oea_gcn_unit_epoch(const oea_gcn_unit *u, float *w, const oea_gcn_unit_buffers *b, double *loss_accum, void *stream);

/* ---------------------------------------------------------------------------------------
 * Graph builders on the device (csrc/graph_build.hip) -- the per-init adjacency construction of the GNN approaches.
 * Inputs: triples int32 [n, 3] (device).  Outputs are sorted by (row, col); their sizes are data dependent: the caller
 * passes buffers of `cap` entries (cap >= 2 * n_tri + n_ent covers every case) and reads *nnz_dev back.  All sums run in
 * a fixed order (stable sort + segmented reduction): two processes build bit-identical operands.  These calls
 * synchronise the stream (they read intermediate counts back): they run once per model init, not in an epoch.
 * ------------------------------------------------------------------------------------- */
/* approaches/alinet.py:155-181: distinct undirected (h, t) pairs as 0/1 entries, + I, D^-1/2 . D^-1/2
 * (preprocess_adj, alinet.py:114-132).  fp64 values like scipy's. */
int oea_build_unweighted_adj(const int32_t *tri, int64_t n_tri, int64_t n_ent, int32_t *row, int32_t *col, double *val,
                             int64_t cap, int64_t *nnz_dev, void *stream);
/* approaches/gcn_align.py:610-640 (r2f / r2if [n_rel] fp64 = distinct heads / tails per triple of a relation),
 * :642-664 (M[(h,t)] += max(r2if, .3), M[(t,h)] += max(r2f, .3); entry of key (a, b) at row b, column a; optional raw
 * adjacency outputs adj_*: NULL to skip) and :566-578 (support = normalize_adj(adj + I) = (A' D^-1/2)^T D^-1/2). */
int oea_build_weighted_adj(const int32_t *tri, int64_t n_tri, int64_t n_ent, int64_t n_rel, double *r2f, double *r2if,
                           int32_t *adj_row, int32_t *adj_col, double *adj_val, int64_t *adj_nnz_dev, int32_t *row,
                           int32_t *col, double *val, int64_t cap, int64_t *nnz_dev, void *stream);
/* approaches/rdgcn.py:45-72 (get_mat + get_sparse_tensor): M[sec, fir] = 1 / sqrt(deg[fir]) / sqrt(deg[sec]) over the
 * symmetric closure of the (h, t) pairs with h != t plus the diagonal, with get_mat's degree rule; values as fp32. */
int oea_build_primal_adj(const int32_t *tri, int64_t n_tri, int64_t n_ent, int32_t *row, int32_t *col, float *val,
                         int64_t cap, int64_t *nnz_dev, void *stream);
/* approaches/rdgcn.py:17-42 + :268-277: out [n_rel, n_rel] fp32 = Jaccard overlap of the relations' head sets + of
 * their tail sets. */
int oea_build_dual_adj(const int32_t *tri, int64_t n_tri, int64_t n_rel, float *out, void *stream);
/* approaches/alinet.py:250-287 (generate_2hop_triples): self-join of `tri` (tail == head, left triple major, matches in
 * table order), rows whose (h, t) is an edge of `full_tri` dropped, the n_cut most frequent (r1, r2) patterns dropped
 * (ties: first appearance in the joined table, i.e. python's stable sort), out = distinct (h, r1 + r2, t) of the kept
 * rows plus (h, 0, h) for their heads, sorted.  stats_host[4] = the reference's four log counts (distinct joined
 * (h, r1, r2, t); patterns; patterns kept; triples out). */
int oea_build_2hop(const int32_t *tri, int64_t n_tri, const int32_t *full_tri, int64_t n_full, int64_t n_ent,
                   int64_t n_rel, int32_t n_cut, int32_t *out, int64_t cap, int64_t *n_out_dev, int64_t *stats_host,
                   void *stream);

/* ---------------------------------------------------------------------------------------
 * Collective group (one process per GPU, RCCL over xGMI) -- no reference counterpart (the reference is single-device,
 * SURVEY F2).  The exchange points of the multi-GPU path for a host that is not Python: reduce-scatter / all-gather of
 * the partitioned step (oea_part_*), int64 / fp64 sums of the row-sharded evaluation's metrics, all-gather of row blocks
 * (argmax, neighbour lists, a graph layer's output rows).  RCCL is dlopen'ed by oea_comm_unique_id / oea_comm_init: a
 * single-GPU process never loads it.  The Python host uses torch.distributed (backend "nccl" = the same RCCL).
 *   rank 0: oea_comm_unique_id(id) -> ship the 128 bytes to the other ranks (any channel) -> every rank, after
 *   hipSetDevice(its GPU): oea_comm_init(id, rank, nranks, &comm).  Calls are asynchronous on `stream`.
 * ------------------------------------------------------------------------------------- */
typedef struct oea_comm *oea_comm_t;
int oea_comm_unique_id(void *id_out_128);
int oea_comm_init(const void *unique_id_128, int32_t rank, int32_t nranks, oea_comm_t *out);
/* A communicator over HOST CALLBACKS instead of RCCL: every collective of the entry points below (and of
 * oea_triple_epoch_range_comm) is handed to `fn`: op = OEA_COMM_*, send / recv = device pointers, count = elements PER RANK
 * (all-gather: elements of every rank's send block; reduce-scatter: elements of every rank's recv block; all-reduce:
 * elements of the buffer, send == recv), dtype = OEA_COMM_F32 / F64 / I64.  The callback must order itself after the work
 * already enqueued on `stream` and leave the result visible to work enqueued after it returns; it returns 0 on success.
 * RCCL needs one GPU per rank: with callbacks over torch.distributed's gloo group the build pool's ONE GPU runs the call path
 * with 2 and 4 ranks (tests/test_partition_gpu.py). */
enum { OEA_COMM_ALLREDUCE = 0, OEA_COMM_ALLGATHER = 1, OEA_COMM_REDUCE_SCATTER = 2 };
enum { OEA_COMM_F32 = 0, OEA_COMM_F64 = 1, OEA_COMM_I64 = 2 };
typedef int (*oea_comm_callback)(void *user, int32_t op, const void *send, void *recv, int64_t count, int32_t dtype, void *stream);
int oea_comm_init_callbacks(int32_t rank, int32_t nranks, oea_comm_callback fn, void *user, oea_comm_t *out);
int oea_comm_destroy(oea_comm_t c);
int32_t oea_comm_rank(oea_comm_t c);
int32_t oea_comm_size(oea_comm_t c);
/* recv [nranks][rows_per_rank, ld] <- every rank's send [rows_per_rank, ld] */
int oea_allgather_rows(oea_comm_t c, const float *send, float *recv, int64_t rows_per_rank, int32_t ld, void *stream);
/* recv [n_per_rank] = sum over ranks of send[rank * n_per_rank ...] (send holds nranks * n_per_rank floats) */
int oea_comm_reduce_scatter_f32(oea_comm_t c, const float *send, float *recv, int64_t n_per_rank, void *stream);
int oea_allreduce_f32(oea_comm_t c, float *buf, int64_t n, void *stream);
int oea_allreduce_f64(oea_comm_t c, double *buf, int64_t n, void *stream);
int oea_allreduce_i64(oea_comm_t c, int64_t *buf, int64_t n, void *stream);
/* the same three collectives for any of the dtypes (the deterministic build exchanges int64 fixed-point gradients) */
int oea_comm_allgather(oea_comm_t c, const void *send, void *recv, int64_t n_per_rank, int32_t dtype, void *stream);
int oea_comm_reduce_scatter(oea_comm_t c, const void *send, void *recv, int64_t n_per_rank, int32_t dtype, void *stream);
int oea_comm_allreduce(oea_comm_t c, void *buf, int64_t n, int32_t dtype, void *stream);
/* All-to-all with per-peer element counts known on the host: peer p receives send[send_displs[p] .. + send_counts[p]) and
 * recv[recv_displs[p] ..] takes recv_counts[p] elements from p.  RCCL: one group of ncclSend / ncclRecv; a callback communicator
 * hands it to the function set by oea_comm_set_alltoallv (same ordering contract as oea_comm_callback). */
typedef int (*oea_comm_alltoallv_callback)(void *user, const void *send, const int64_t *send_counts, const int64_t *send_displs,
                                           void *recv, const int64_t *recv_counts, const int64_t *recv_displs, int32_t dtype, void *stream);
int oea_comm_set_alltoallv(oea_comm_t c, oea_comm_alltoallv_callback fn);
int oea_comm_alltoallv(oea_comm_t c, const void *send, const int64_t *send_counts, const int64_t *send_displs, void *recv,
                       const int64_t *recv_counts, const int64_t *recv_displs, int32_t dtype, void *stream);

/* oea_triple_epoch_range_comm with the BOUNDARY-ROW ("halo") exchange (BASELINE.json north_star: "all-gather of boundary
 * embeddings"): instead of every owned row (reduce-scatter + all-gather of [E, ld] per step) a step moves only the rows its batch
 * refers to.  Every rank derives from the epoch's positives and negatives (drawn ahead, the same Philox streams everywhere) the
 * sorted list of rows each rank's share of each step refers to, per owner (owner = id mod world) -- no index travels and all
 * message sizes are known after ONE host read of the [steps][world][world] counts per call.  Per step: GRAD -> all-to-all of the
 * gradient rows (+ flag) to their owners, added into the owner's scratch (exact in the fixed-point build: the G-rank job is the
 * single-GPU job bit for bit) -> relation rows all-reduced -> optimiser on the owned rows -> all-to-all of the current values of
 * the rows the next step's readers refer to.  The last step of the range ends with the dense all-gather of the owned rows
 * (upd / all as above), so outside the call every rank holds the whole table.  TransE / TransH scores, SGD / Adagrad.
 *   halo_ws: oea_halo_workspace_bytes(n_ent, world, step_end - step_begin or more, largest batch, k) device bytes;
 *   buf_a, buf_b: two exchange buffers of oea_halo_buffer_bytes(...) device bytes each;
 *   stats_host (may be NULL): int64 [4] = bytes pushed (gradient rows sent), bytes pulled (rows received), largest number of
 *   rows sent in a step, steps run. */
size_t oea_halo_workspace_bytes(int64_t n_ent, int32_t world, int32_t steps, int64_t max_batch, int32_t k);
/* the plan alone (what oea_triple_epoch_range_halo computes first): counts_host [step_end - step_begin][world][world] = distinct entity
 * rows rank r's share of step s refers to that rank o owns; lists_host (may be NULL) [steps][world][*cap_out] = the lists (local row
 * indices j, entity id = j * world + o; owner-major, ascending).  neg_all = the epoch's negatives [rows * k, 3] (NULL when k = 0). */
int oea_halo_plan(const int32_t *pos_all, const int32_t *neg_all, int32_t k, const int64_t *offsets_host, const int64_t *offsets_dev,
                  int32_t steps, int32_t step_begin, int32_t step_end, int64_t n_ent, int32_t world, void *halo_ws, size_t halo_ws_bytes,
                  int32_t *counts_host, int32_t *lists_host, int64_t *cap_out, void *stream);
size_t oea_halo_buffer_bytes(int64_t n_ent, int32_t world, int64_t max_batch, int32_t k, int32_t ld);
int oea_triple_epoch_range_halo(oea_comm_t comm, const oea_epoch *e, int32_t step_begin, int32_t step_end, void *halo_ws,
                                size_t halo_ws_bytes, void *buf_a, void *buf_b, size_t buf_bytes, void *rel_x, float *upd, float *all,
                                int64_t *stats_host, void *stream);

/* Phase times of oea_triple_epoch_range_comm: between _begin and _end every step records HIP events at its phase boundaries
 * on the call's stream; _end waits for the last one and returns the summed milliseconds per phase
 * (GRAD | pack | reduce-scatter + relation all-reduce | apply | all-gather | unpack; for oea_triple_epoch_range_halo: GRAD | pack |
 * gradient all-to-all + relation all-reduce | add + apply | row all-to-all (or the closing all-gather) | unpack) and the number of
 * steps recorded. */
enum { OEA_COMM_PHASES = 6 };
int oea_comm_profile_begin(oea_comm_t c);
int oea_comm_profile_end(oea_comm_t c, double *phase_ms /* [OEA_COMM_PHASES] */, int32_t *steps);

#ifdef __cplusplus
}
#endif
#endif /* OPENEA_HIP_H */
