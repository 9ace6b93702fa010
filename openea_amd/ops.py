"""Thin typed wrappers over the C ABI (include/openea_hip.h).

PyTorch is plumbing here: device allocations (``torch.empty(..., device='cuda')``), the
current HIP stream and ``torch.distributed``.  All arithmetic happens inside
libopenea_hip.so; nothing in this module computes on the CPU.
"""
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib
from ._lib import LOSS_KIND, METRIC, OPT_KIND, OpenEAHipError, RotateCfg, StepCfg, check


def lib():
    return _lib.load(require_device=True)


def _p(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device-resident contiguous tensor required"
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def pad4(d):
    return (int(d) + 3) // 4 * 4


def device(index=None):
    lib()
    return torch.device('cuda', torch.cuda.current_device() if index is None else index)


# -------------------------------------------------------------------------------------------
# tables
# -------------------------------------------------------------------------------------------


def to_table(array, ld=None, dev=None):
    """host [n, d] (numpy / list) -> device fp32 [n, ld] zero-padded (ld % 4 == 0)."""
    a = np.ascontiguousarray(np.asarray(array, dtype=np.float32))
    assert a.ndim == 2
    n, d = a.shape
    ld = pad4(d) if ld is None else ld
    t = torch.zeros((n, ld), dtype=torch.float32, device=dev or device())
    if n:
        t[:, :d].copy_(torch.from_numpy(a), non_blocking=False)
    return t


def to_vec(array, dev=None):
    """host 1-D float array -> device fp32 vector."""
    a = np.ascontiguousarray(np.asarray(array, dtype=np.float32)).reshape(-1)
    return torch.from_numpy(a).to(dev or device())


def to_ids(array, dev=None):
    a = np.ascontiguousarray(np.asarray(array, dtype=np.int32))
    return torch.from_numpy(a).to(dev or device())


def gather_rows(table, dim, ids, normalize=False, out_ld=None):
    """tf.nn.embedding_lookup(l2_normalize?(table), ids) -> device [n, out_ld]."""
    n = ids.numel()
    out_ld = pad4(dim) if out_ld is None else out_ld
    out = torch.empty((n, out_ld), dtype=torch.float32, device=table.device)
    check(lib().oea_gather_rows(_p(table), dim, table.shape[1], _p(ids), n, int(bool(normalize)),
                                _p(out), out_ld, _stream()))
    return out


def normalize_rows_(table, dim, sklearn=True):
    check(lib().oea_normalize_rows(_p(table), table.shape[0], dim, table.shape[1], int(bool(sklearn)), _stream()))
    return table


# -------------------------------------------------------------------------------------------
# translational step
# -------------------------------------------------------------------------------------------


SCORE_TRANSE, SCORE_TRANSH, SCORE_TRANSD = 0, 1, 2


def make_step_cfg(loss='limited', loss_norm='L2', margin=0.0, pos_margin=0.0, neg_margin=0.0,
                  balance=1.0, ent_l2_norm=True, rel_l2_norm=True, optimizer='Adagrad', lr=0.01,
                  neg_group_k=0, normal=None, normal_acc=None, transfer_bases=None):
    """neg_group_k = k when the negatives are laid out as the device sampler writes them
    (neg[p*k:(p+1)*k] corrupt pos p); 0 for arbitrary lists.
    normal (+ normal_acc for Adagrad): device [n_rel, ld] normal_vector table -> TransH scoring.
    transfer_bases = (n_ent, n_rel): TransD scoring on stacked tables (rows [n, 2n) hold the transfer vectors)."""
    assert normal is None or transfer_bases is None
    score = SCORE_TRANSH if normal is not None else (SCORE_TRANSD if transfer_bases is not None else SCORE_TRANSE)
    eb, rb = transfer_bases if transfer_bases is not None else (0, 0)
    # tf.train defaults: AdamOptimizer(beta1=0.9, beta2=0.999, epsilon=1e-8), AdadeltaOptimizer(rho=0.95, epsilon=1e-8)
    b1 = 0.95 if optimizer == 'Adadelta' else 0.9
    cfg = StepCfg(LOSS_KIND[loss], 1 if loss_norm == 'L1' else 0, float(margin), float(pos_margin),
                  float(neg_margin), float(balance), int(bool(ent_l2_norm)), int(bool(rel_l2_norm)),
                  OPT_KIND[optimizer], float(lr), int(neg_group_k), score,
                  None if normal is None else normal.data_ptr(), None if normal_acc is None else normal_acc.data_ptr(),
                  int(eb), int(rb), b1, 0.999, 1e-8, 0)
    cfg._keep = (normal, normal_acc)
    return cfg


def scratch_dtype():
    """element type of the step's gradient scratch, its touched flags and the partition's exchange buffers: fp32, or int64
    fixed point in the deterministic build (OEA_STEP_DETERMINISTIC=1 -> libopenea_hip_det.so, csrc/common.h)"""
    return torch.int64 if lib().oea_step_scratch_elem_bytes() == 8 else torch.float32


def deterministic():
    return lib().oea_step_scratch_elem_bytes() == 8


def step_workspace(n_ent, n_rel, ld, dev=None):
    nbytes = lib().oea_step_workspace_bytes(n_ent, n_rel, ld)
    return torch.zeros(nbytes, dtype=torch.uint8, device=dev or device())


PHASE_BOTH, PHASE_GRAD, PHASE_APPLY = 0, 1, 2


def triple_step(ent, ent_acc, rel, rel_acc, dim, pos, neg, cfg, workspace, loss_accum, phase=PHASE_BOTH):
    """One optimiser step in place; the batch loss is added to `loss_accum` (device f64[1]).
    phase: PHASE_GRAD / PHASE_APPLY split the step at its exchange point (data parallelism)."""
    n_neg = 0 if neg is None else neg.shape[0]
    check(lib().oea_triple_step_phase(_p(ent), _p(ent_acc), ent.shape[0], _p(rel), _p(rel_acc), rel.shape[0],
                                      dim, ent.shape[1], _p(pos), pos.shape[0], _p(neg), n_neg,
                                      C.byref(cfg), _p(workspace), _p(loss_accum), int(phase), _stream()))


# ---- RotatE (fp64) --------------------------------------------------------------------------------------------
def to_table64(array, dev=None):
    """host [n, d] -> device fp64 [n, ld] zero-padded (ld % 4 == 0)."""
    a = np.ascontiguousarray(np.asarray(array, dtype=np.float64))
    n, d = a.shape
    t = torch.zeros((n, pad4(d)), dtype=torch.float64, device=dev or device())
    if n:
        t[:, :d].copy_(torch.from_numpy(a))
    return t


def make_rotate_cfg(gamma, dim, ent_l2_norm=True, rel_l2_norm=False, optimizer='Adam', lr=0.01, beta1=0.9, beta2=0.999,
                    eps=1e-8, epsilon=2.0, neg_loss_div=0):
    """bootea_rotate.py:29-33,90: embedding_range = (gamma + epsilon) / dim, phase = rel / (embedding_range / pi).
    neg_loss_div = k > 1: the negatives' half of the loss divided by k (the plain RotatE, rotate.py:81); 0 or 1: undivided."""
    rng = (float(gamma) + float(epsilon)) / dim
    return RotateCfg(float(gamma), 3.14159265358979323846 / rng, float(lr), float(beta1), float(beta2), float(eps), 0,
                     int(bool(ent_l2_norm)), int(bool(rel_l2_norm)), OPT_KIND[optimizer], int(neg_loss_div))


def rotate_workspace(n_ent, n_rel, ld, dev=None):
    return torch.zeros(lib().oea_rotate_workspace_bytes(n_ent, n_rel, ld), dtype=torch.uint8, device=dev or device())


def rotate_exchange_view(workspace, n_ent, n_rel, ld):
    """fp64 view of the workspace prefix that data-parallel ranks sum between PHASE_GRAD and PHASE_APPLY."""
    n = lib().oea_rotate_exchange_doubles(n_ent, n_rel, ld)
    return workspace[: n * 8].view(torch.float64)


def rotate_state(table, optimizer):
    """optimiser state of one fp64 table: Adagrad accumulator (0.1), Adam [m ; v] (zeros), None for SGD."""
    if optimizer == 'Adagrad':
        return torch.full_like(table, 0.1)
    if optimizer == 'Adam':
        return torch.zeros((2,) + tuple(table.shape), dtype=torch.float64, device=table.device)
    return None


def rotate_step(ent, ent_state, rel, rel_state, dim, pos, neg, neg_group_k, cfg, workspace, loss_accum, phase=PHASE_BOTH):
    """One RotatE optimiser step in place (ent: fp64 [2E, ld], re rows then im rows).  cfg.t must hold the 1-based
    step count of this optimiser when it is Adam."""
    n_neg = 0 if neg is None else neg.shape[0]
    check(lib().oea_rotate_step(_p(ent), _p(ent_state), ent.shape[0] // 2, _p(rel), _p(rel_state), rel.shape[0], dim,
                                ent.shape[1], _p(pos), pos.shape[0], _p(neg), n_neg, int(neg_group_k), C.byref(cfg),
                                _p(workspace), _p(loss_accum), int(phase), _stream()))


def rotate_lookup(ent, dim, ids, part_norm=True, sum_norm=False):
    """fp32 [n, pad4(dim)] block of l2n?(l2n?(re[ids]) + l2n?(im[ids])) for the evaluation kernels."""
    n = ent.shape[0] // 2 if ids is None else ids.numel()
    out = torch.empty((n, pad4(dim)), dtype=torch.float32, device=ent.device)
    check(lib().oea_rotate_lookup(_p(ent), ent.shape[0] // 2, dim, ent.shape[1], _p(ids), n, int(bool(part_norm)),
                                  int(bool(sum_norm)), _p(out), out.shape[1], _stream()))
    return out


def step_scatter_ent_rows(workspace, n_ent, n_rel, ld, ids, src):
    """grad_scratch[ids[i]] += src[i] (+ touched flags): gradients w.r.t. normalised entity rows
    computed outside the fused step (MTransE mapping loss)."""
    check(lib().oea_step_scatter_ent_rows(_p(workspace), n_ent, n_rel, ld, _p(ids), ids.numel(), _p(src),
                                          src.shape[1], _stream()))


def mapping_step(ent, dim, ent_l2_norm, ids1, ids2, mapping, mapping_acc, alpha, lr, optimizer, workspace, n_ent, n_rel,
                 loss_accum, work=None):
    """MTransE mapping step (oea_mapping_step): updates `mapping` in place and adds the entity-row gradients into
    the step workspace's scratch; follow with triple_step(..., empty, phase=PHASE_APPLY)."""
    n = ids1.numel()
    need = lib().oea_mapping_workspace_floats(n, ent.shape[1], dim)
    if work is None or work.numel() < need:
        work = torch.empty(need, dtype=torch.float32, device=ent.device)
    eg, et = C.c_void_p(), C.c_void_p()
    check(lib().oea_step_entity_scratch(_p(workspace), n_ent, n_rel, ent.shape[1], C.byref(eg), C.byref(et)))
    check(lib().oea_mapping_step(_p(ent), ent.shape[1], dim, int(bool(ent_l2_norm)), _p(ids1), _p(ids2), n, _p(mapping),
                                 _p(mapping_acc), float(alpha), float(lr), OPT_KIND[optimizer], eg, et, _p(work),
                                 _p(loss_accum), _stream()))
    return work


def mapping_epoch(ent, ent_acc, rel, rel_acc, dim, ent_l2_norm, batches, mapping, mapping_acc, alpha, lr, optimizer, cfg, workspace,
                  mapping_loss, step_loss, work=None):
    """a whole MTransE mapping epoch with one call (oea_mapping_epoch): batches device int32 [steps, 2, n]."""
    steps, _, n = batches.shape
    need = lib().oea_mapping_workspace_floats(n, ent.shape[1], dim)
    if work is None or work.numel() < need:
        work = torch.empty(need, dtype=torch.float32, device=ent.device)
    check(lib().oea_mapping_epoch(_p(ent), _p(ent_acc), ent.shape[0], _p(rel), _p(rel_acc), rel.shape[0], dim, ent.shape[1],
                                  int(bool(ent_l2_norm)), _p(batches), int(steps), int(n), _p(mapping), _p(mapping_acc), float(alpha),
                                  float(lr), OPT_KIND[optimizer], C.byref(cfg), _p(workspace), _p(work), _p(mapping_loss),
                                  _p(step_loss), _stream()))
    return work


# ---- SEA -------------------------------------------------------------------------------------------------------
SEA_MAX_DIM = 128


def _sea_work(n_l, n_u, ld, dim, work, dev):
    need = lib().oea_sea_mapping_workspace_floats(int(n_l), int(n_u), int(ld), int(dim))
    if work is None or work.numel() < need:
        work = torch.empty(need, dtype=torch.float32, device=dev)
    return work


def sea_mapping_step(ent, dim, ids_l1, ids_l2, ids_u1, ids_u2, m1, m2, m_state, alpha_1, alpha_2, cfg, workspace, n_ent, n_rel,
                     loss_accum, work=None):
    """SEA's mapping step (oea_sea_mapping_step): updates `m1` / `m2` (and Adam's `m_state` [4, d, d]) in place and adds the
    entity-row gradients into the step workspace's scratch; follow with triple_step(..., empty, phase=PHASE_APPLY) under the
    same cfg.  ids_l* / ids_u*: device int32 vectors (either pair may be empty)."""
    n_l, n_u = ids_l1.numel(), ids_u1.numel()
    assert ids_l2.numel() == n_l and ids_u2.numel() == n_u
    work = _sea_work(n_l, n_u, ent.shape[1], dim, work, ent.device)
    eg, et = C.c_void_p(), C.c_void_p()
    check(lib().oea_step_entity_scratch(_p(workspace), n_ent, n_rel, ent.shape[1], C.byref(eg), C.byref(et)))
    check(lib().oea_sea_mapping_step(_p(ent), ent.shape[1], dim, _p(ids_l1), _p(ids_l2), n_l, _p(ids_u1), _p(ids_u2), n_u, _p(m1),
                                     _p(m2), _p(m_state), float(alpha_1), float(alpha_2), C.byref(cfg), eg, et, _p(work),
                                     _p(loss_accum), _stream()))
    return work


def sea_mapping_epoch(ent, ent_acc, rel, rel_acc, dim, batches, n_l, n_u, m1, m2, m_state, alpha_1, alpha_2, cfg, workspace,
                      mapping_loss, step_loss, work=None):
    """a whole SEA mapping epoch with one call (oea_sea_mapping_epoch): batches device int32 [steps, 2 n_l + 2 n_u], every row
    [l1 | l2 | u1 | u2]; cfg.opt_t = the 1-based count of the epoch's first step."""
    steps = batches.shape[0]
    assert batches.dim() == 2 and batches.shape[1] == 2 * (n_l + n_u)
    work = _sea_work(n_l, n_u, ent.shape[1], dim, work, ent.device)
    check(lib().oea_sea_mapping_epoch(_p(ent), _p(ent_acc), ent.shape[0], _p(rel), _p(rel_acc), rel.shape[0], dim, ent.shape[1],
                                      _p(batches), int(steps), int(n_l), int(n_u), _p(m1), _p(m2), _p(m_state), float(alpha_1),
                                      float(alpha_2), C.byref(cfg), _p(workspace), _p(work), _p(mapping_loss), _p(step_loss),
                                      _stream()))
    return work


# ---- TransR ----------------------------------------------------------------------------------------------------
TRANSR_MAX_DIM = 128


def transr_workspace(n_ent, n_rel, dim, max_pos, dev=None):
    """scratch of oea_transr_step for batches of at most max_pos pairs (no initialisation needed)"""
    return torch.empty(lib().oea_transr_workspace_bytes(n_ent, n_rel, dim, max_pos), dtype=torch.uint8, device=dev or device())


def transr_step(ent, ent_acc, rel, rel_acc, rel_matrix, rel_matrix_acc, dim, pos, neg, cfg, workspace, transr_ws, loss_accum):
    """One TransR optimiser step in place (oea_transr_step): rel_matrix device fp32 [R, dim*dim] (+ its Adagrad accumulator),
    ent / rel as for triple_step, pos / neg int32 [n, 3] paired row by row; the batch loss is added to `loss_accum`."""
    assert rel_matrix.shape == (rel.shape[0], dim * dim) and rel_matrix.dtype == torch.float32
    n_neg = 0 if neg is None else neg.shape[0]
    check(lib().oea_transr_step(_p(ent), _p(ent_acc), ent.shape[0], _p(rel), _p(rel_acc), rel.shape[0], _p(rel_matrix),
                                _p(rel_matrix_acc), dim, ent.shape[1], _p(pos), pos.shape[0], _p(neg), n_neg, C.byref(cfg),
                                _p(workspace), _p(transr_ws), _p(loss_accum), _stream()))


# ---- HolE / SimplE / DistMult -----------------------------------------------------------------------------------
SEMANTIC_HOLE, SEMANTIC_SIMPLE, SEMANTIC_DISTMULT = 0, 1, 2
SEMANTIC_MAX_DIM = 128


def semantic_step(model, ent, ent_acc, rel, rel_acc, dim, pos, neg, cfg, workspace, loss_accum):
    """One HolE / SimplE / DistMult optimiser step in place (oea_semantic_step): model SEMANTIC_HOLE, SEMANTIC_SIMPLE (stacked
    tables: ent = [H; T], rel = [R1; R2]) or SEMANTIC_DISTMULT; neg [n * k, 3] with neg[p*k:(p+1)*k] the corruptions of pos p,
    k = cfg.neg_group_k; the batch loss (DistMult: the mean over the n * (k + 1) labelled triples) is added to `loss_accum`."""
    n_neg = 0 if neg is None else neg.shape[0]
    check(lib().oea_semantic_step(int(model), _p(ent), _p(ent_acc), ent.shape[0], _p(rel), _p(rel_acc), rel.shape[0], dim,
                                  ent.shape[1], _p(pos), pos.shape[0], _p(neg), n_neg, C.byref(cfg), _p(workspace),
                                  _p(loss_accum), _stream()))


# ---- JAPE -------------------------------------------------------------------------------------------------------
JAPE_MAX_DIM = 128


def jape_step(ent, ent_acc, rel, rel_acc, dim, pos, neg, neg_alpha, cfg, workspace, loss_accum):
    """One JAPE triple step in place (oea_jape_step): loss = sum_pos |h + r - t|^2 - neg_alpha sum_neg |h + r - t|^2 on the rows
    normalised by cfg's flags; neg [n * k, 3] with neg[p*k:(p+1)*k] the corruptions of pos p, k = cfg.neg_group_k; the batch
    SUM is added to `loss_accum`."""
    n_neg = 0 if neg is None else neg.shape[0]
    check(lib().oea_jape_step(_p(ent), _p(ent_acc), ent.shape[0], _p(rel), _p(rel_acc), rel.shape[0], dim, ent.shape[1], _p(pos),
                              pos.shape[0], _p(neg), n_neg, float(neg_alpha), C.byref(cfg), _p(workspace), _p(loss_accum),
                              _stream()))


# ---- MultiKE ----------------------------------------------------------------------------------------------------
MULTIKE_MAX_DIM = 128
MULTIKE_VARS = ("gamma", "beta", "K1", "b1", "K2", "b2", "W", "bd")
MULTIKE_ROWS_CROSS, MULTIKE_ROWS_PULL, MULTIKE_ROWS_WSOFT = 0, 1, 2


def multike_cnn_shapes(dim, ld=None):
    """shapes of the eight variables of one parameter set, in the order of MULTIKE_VARS (W with row stride ld)"""
    ld = pad4(dim) if ld is None else ld
    return ((dim,), (dim,), (2, 4, 1, 2), (2,), (2, 4, 2, 2), (2,), (4 * dim, ld), (dim,))


def multike_cnn_workspace(dim, ld, max_n, dev=None):
    """workspace of multike_cnn_step for batches of up to max_n positives (no initialisation needed)"""
    n = lib().oea_multike_cnn_workspace_bytes(int(dim), int(ld), int(max_n))
    if n == 0:
        raise OpenEAHipError("oea_multike_cnn_workspace_bytes: dim=%d ld=%d max_n=%d" % (dim, ld, max_n))
    ws = torch.zeros(n, dtype=torch.uint8, device=dev or device())
    ws._shape = (int(dim), int(ld), int(max_n))
    return ws


def multike_cnn_grads(workspace, net=0):
    """views of the eight dense fp32 parameter gradients of net `net` that the last multike_cnn_step left in the workspace"""
    dim, ld, max_n = workspace._shape
    ptrs = (C.c_void_p * 8)()
    check(lib().oea_multike_cnn_grads(_p(workspace), dim, ld, max_n, int(net), ptrs))
    out = []
    for ptr, shape in zip(ptrs, multike_cnn_shapes(dim, ld)):
        off = ptr - workspace.data_ptr()
        out.append(workspace[off:off + 4 * int(np.prod(shape))].view(torch.float32).view(shape))
    return out


def multike_net(params, ent, step_ws, n_rel_ws, weighted=False, ent_l2_norm=True, factor=1.0):
    """one net of multike_cnn_step: its eight variables (MULTIKE_VARS), its entity table and that table's step workspace of
    (ent rows, n_rel_ws) rows"""
    assert len(params) == 8 and all(t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 for t in list(params) + [ent])
    return dict(params=list(params), ent=ent, ws=step_ws, n_rel_ws=int(n_rel_ws), weighted=bool(weighted), l2n=bool(ent_l2_norm),
                factor=float(factor))


def multike_cnn_step(nets, attr, lit, dim, batch, attr_weight, lr, workspace, loss_accum, phase=PHASE_BOTH):
    """The attribute CNN of MultiKE on batch int32 [n, 3] = (entity, attribute, literal) for 1 or 2 nets (multike_net) that share
    attr [n_attr, ld] (raw) and lit [n_lit, ld] (constant); attr_weight float [n_attr] weights the positives of the weighted nets.
    PHASE_GRAD: parameter gradients through multike_cnn_grads, row gradients in the nets' step workspaces (the attribute rows in
    net 0's); PHASE_BOTH: SGD with lr on the parameters as well.  triple_step(..., empty, phase=PHASE_APPLY) on each table pair
    finishes the step.  The loss of all nets is added to `loss_accum`."""
    wdim, ld, max_n = workspace._shape
    assert wdim == dim and attr.shape[1] == ld and lit.shape[1] == ld and batch.dtype == torch.int32 and batch.shape[1] == 3
    arr = (_lib.MultiKENet * len(nets))()
    for s, n in zip(arr, nets):
        assert n["ent"].shape[1] == ld and n["params"][6].shape == (4 * dim, ld)
        for i, t in enumerate(n["params"]):
            s.p[i] = t.data_ptr()
        s.ent, s.step_workspace, s.n_rel_ws = n["ent"].data_ptr(), n["ws"].data_ptr(), n["n_rel_ws"]
        s.weighted, s.ent_l2_norm, s.factor = int(n["weighted"]), int(n["l2n"]), n["factor"]
    check(lib().oea_multike_cnn_step(arr, len(nets), nets[0]["ent"].shape[0], _p(attr), attr.shape[0], _p(lit), lit.shape[0], dim, ld,
                                     _p(batch), batch.shape[0], _p(attr_weight), float(lr), _p(workspace), max_n, _p(loss_accum),
                                     int(phase), _stream()))


def multike_rows(kind, table_a, ws_a, n_rel_a, table_b, ws_b, n_rel_b, rel, dim, items, coef, loss_accum, rel_weight=None,
                 a_l2_norm=True, b_l2_norm=True, rel_l2_norm=True, rel_side=0):
    """MultiKE's row-wise terms (oea_multike_rows): MULTIKE_ROWS_CROSS coef |A[h] + rel[r] - B[t]|^2, MULTIKE_ROWS_PULL
    coef |A[e] - B[e]|^2 (ws_b None: B is constant), MULTIKE_ROWS_WSOFT coef rel_weight[r] softplus(|A[h] + rel[r] - B[t]|^2);
    gradients into the step workspaces, the relation rows' into ws_a (rel_side 0) or ws_b (rel_side 1)."""
    assert items.dtype == torch.int32
    n = items.shape[0]
    check(lib().oea_multike_rows(int(kind), _p(table_a), _p(ws_a), int(n_rel_a), int(bool(a_l2_norm)), _p(table_b), _p(ws_b),
                                 int(n_rel_b), int(bool(b_l2_norm)), _p(rel), int(bool(rel_l2_norm)), table_a.shape[0], int(rel_side),
                                 dim, table_a.shape[1], _p(items), n, _p(rel_weight), float(coef), _p(loss_accum), _stream()))


# ---- AttrE ------------------------------------------------------------------------------------------------------
ATTRE_MAX_DIM = 128
ATTRE_MAX_LITERAL_LEN = 32
ATTRE_PATH_AUTO, ATTRE_PATH_LDS, ATTRE_PATH_ATOMIC = 0, 1, 2


def attre_lds_chars(ld):
    """the largest character table [C, ld] whose gradient slab the character step still sums in LDS (oea_attre_lds_chars; half as
    many in the deterministic build, whose slab holds int64)"""
    return int(lib().oea_attre_lds_chars(int(ld)))


def attre_char_workspace(n_chars, ld, max_pos, dev=None):
    nbytes = lib().oea_attre_char_workspace_bytes(int(n_chars), int(ld), int(max_pos))
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev or device())


def attre_check(err_flag):
    """what the check kernel of attre_char_step found in device memory (reads the flag: a host wait)"""
    e = int(err_flag.item())
    if e:
        raise OpenEAHipError("AttrE's character step refused its device arguments (nothing was written):%s%s"
                             % (" a character id lies outside the character table;" if e & 1 else "",
                                " a value, entity or attribute id lies outside its table" if e & 2 else ""))


def attre_char_step(ent_ce, ent_acc, attr, attr_acc, chars, char_acc, dim, value_chars, pos, neg_heads, char_l2_norm, cfg, workspace,
                    char_ws, err_flag, loss_accum, char_path=ATTRE_PATH_AUTO, n_slabs=0):
    """One character step of AttrE in place (oea_attre_char_step): pos int32 [n, 3] = (entity, attribute, row of value_chars),
    neg_heads int32 [n * k] with neg_heads[p*k:(p+1)*k] the corrupted heads of pos p, k = cfg.neg_group_k; value_chars int32
    [n_values, literal_len]; the batch sum is added to `loss_accum`.  err_flag: device int32 [1], zeroed (attre_check reads it)."""
    n_neg = 0 if neg_heads is None else neg_heads.numel()
    check(lib().oea_attre_char_step(_p(ent_ce), _p(ent_acc), ent_ce.shape[0], _p(attr), _p(attr_acc), attr.shape[0], _p(chars),
                                    _p(char_acc), chars.shape[0], dim, ent_ce.shape[1], _p(value_chars), value_chars.shape[0],
                                    value_chars.shape[1], _p(pos), pos.shape[0], _p(neg_heads), n_neg, int(bool(char_l2_norm)),
                                    int(char_path), int(n_slabs), C.byref(cfg), _p(workspace), _p(char_ws), char_ws.numel(),
                                    _p(err_flag), _p(loss_accum), _stream()))


def attre_sample_heads(pos, n_split, k, entity_list0, ent_pos0, entity_list1, ent_pos1, seed, step, pos_offset=0, out=None):
    """head-only negatives of AttrE's attribute triples (oea_attre_sample_heads): rows [0, n_split) of pos draw from entity_list0,
    the rest from entity_list1, never the positive's own head -> device int32 [n * k]"""
    n = pos.shape[0]
    if out is None:
        out = torch.empty(n * k, dtype=torch.int32, device=pos.device)
    assert out.dtype == torch.int32 and out.numel() >= n * k
    n_ent = (ent_pos0 if ent_pos0 is not None else ent_pos1).numel()
    check(lib().oea_attre_sample_heads(_p(pos), n, int(n_split), int(k), _p(entity_list0),
                                       0 if entity_list0 is None else entity_list0.numel(), _p(ent_pos0), _p(entity_list1),
                                       0 if entity_list1 is None else entity_list1.numel(), _p(ent_pos1), n_ent,
                                       int(seed) & (2 ** 64 - 1), int(step) & 0xFFFFFFFF, int(pos_offset) & 0xFFFFFFFF, _p(out), _stream()))
    return out[:n * k]


def attre_joint_epoch(ent, ent_acc, ent_ce, ent_ce_acc, dim, ent_l2_norm, optimizer, lr, steps, loss_accum, row_count=None):
    """`steps` joint steps of AttrE in one pass over both entity tables (oea_attre_joint_epoch); loss_accum: device f64 [steps];
    row_count: device int32 [rows], how often the step's entity list names a row (None: once each)"""
    assert loss_accum.dtype == torch.float64 and loss_accum.numel() >= steps
    assert row_count is None or (row_count.dtype == torch.int32 and row_count.numel() == ent.shape[0])
    check(lib().oea_attre_joint_epoch(_p(ent), _p(ent_acc), _p(ent_ce), _p(ent_ce_acc), _p(row_count), ent.shape[0], dim, ent.shape[1],
                                      int(bool(ent_l2_norm)), OPT_KIND[optimizer], float(lr), int(steps), _p(loss_accum), _stream()))


def sample_distinct(n, m, seed, step, out=None, dev=None):
    """m distinct elements of [0, n) as a pure function of (seed, step) (oea_sample_distinct) -> device int32 [m]"""
    if out is None:
        out = torch.empty(max(int(m), 0), dtype=torch.int32, device=dev or device())
    assert out.dtype == torch.int32 and out.numel() >= m
    check(lib().oea_sample_distinct(int(n), int(m), int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1), _p(out), _stream()))
    return out[:m]


def sim_csr(e1, e2, dim, threshold, block_rows=4096):
    """The entries >= threshold of e1 . e2^T as a CSR -> (indptr int64 [n1 + 1], col int32 [nnz] ascending within a row, val fp32
    [nnz]); the dense matrix exists one block of `block_rows` rows at a time (oea_sim_csr_count / oea_sim_csr_fill).  Reads nnz
    back once."""
    n1, n2 = e1.shape[0], e2.shape[0]
    block_rows = max(1, min(int(block_rows), n1))
    buf = torch.empty((block_rows, n2), dtype=torch.float32, device=e1.device)
    indptr = torch.zeros(n1 + 1, dtype=torch.int64, device=e1.device)
    check(lib().oea_sim_csr_count(_p(e1), n1, e1.shape[1], _p(e2), n2, e2.shape[1], dim, float(threshold), block_rows, _p(buf),
                                  _p(indptr), _stream()))
    nnz = int(indptr[n1].item())
    col = torch.zeros(max(nnz, 1), dtype=torch.int32, device=e1.device)
    val = torch.zeros(max(nnz, 1), dtype=torch.float32, device=e1.device)
    mismatch = torch.zeros(1, dtype=torch.int32, device=e1.device)
    check(lib().oea_sim_csr_fill(_p(e1), n1, e1.shape[1], _p(e2), n2, e2.shape[1], dim, float(threshold), block_rows, _p(buf),
                                 _p(indptr), _p(col), _p(val), _p(mismatch), _stream()))
    if int(mismatch.item()) != 0:
        raise OpenEAHipError("sim_csr: %d rows kept another number of entries in the fill pass than in the count pass"
                             % int(mismatch.item()))
    return indptr, col[:nnz], val[:nnz]


def jape_sim_loss(ent, dim, ref1_ids, ref2_ids, indptr, col, val, rows, beta, loss_accum):
    """loss_accum += beta sum_i |l2n(ent)[ref1_ids[rows[i]]] - l2n(sum_j val_ij l2n(ent)[ref2_ids[col_ij]])|^2 over the CSR rows
    `rows` (oea_jape_sim_loss); writes nothing else."""
    assert indptr.numel() == ref1_ids.numel() + 1
    if col.numel() == 0:              # an empty matrix: the call wants pointers all the same and reads nothing through them
        col, val = torch.zeros(1, dtype=torch.int32, device=ent.device), torch.zeros(1, dtype=torch.float32, device=ent.device)
    check(lib().oea_jape_sim_loss(_p(ent), ent.shape[0], dim, ent.shape[1], _p(ref1_ids), ref1_ids.numel(), _p(ref2_ids),
                                  ref2_ids.numel(), _p(indptr), _p(col), _p(val),
                                  _p(rows), rows.numel(), float(beta), _p(loss_accum), _stream()))


# ---- IMUSE: string similarity (csrc/lcs_sim.hip) ----------------------------------------------------------------------
class StringPool:
    """The distinct strings of one KG side for oea_lcs_ratio_pairs / oea_attr_sim_records: int32 code points back to back (UTF-32:
    the reference compares the elements of a str) + int64 offsets, on the device.  Strings are taken as they come: no strip, no
    lower-casing.  `ids(strings)` -> their indices (int32)."""

    def __init__(self, strings, dev=None):
        self.index = {}
        for s in strings:
            if s not in self.index:
                self.index[s] = len(self.index)
        parts = [np.frombuffer(s.encode('utf-32-le', 'surrogatepass'), dtype='<u4').astype(np.int32) for s in self.index]
        self.lengths = np.array([len(p) for p in parts], np.int64)
        self.n_str, self.n_cp = len(parts), int(self.lengths.sum())
        self.max_len = int(self.lengths.max()) if parts else 0
        off = np.zeros(self.n_str + 1, np.int64)
        np.cumsum(self.lengths, out=off[1:])
        cp = np.concatenate(parts) if self.n_cp else np.zeros(1, np.int32)            # never a null pointer
        dev = dev or device()
        self.cp, self.off = torch.from_numpy(cp).to(dev), torch.from_numpy(off).to(dev)

    def ids(self, strings):
        return np.array([self.index[s] for s in strings], np.int32)

    def _args(self):
        return _p(self.cp), _p(self.off), self.n_str, self.n_cp


def _lcs_workspace(pool1, pool2):
    max_len = max(pool1.max_len, pool2.max_len)
    return max_len, torch.empty(max(lib().oea_lcs_workspace_ints(max_len), 1), dtype=torch.int32, device=pool1.cp.device)


def lcs_check(err_flag):
    """what the check kernels of the two calls below found in device memory (reads the flag: a host wait)"""
    e = int(err_flag.item())
    if e:
        raise OpenEAHipError("string similarity refused its device arguments (nothing was written):%s%s"
                             % (" a pool's offsets do not start at 0, decrease, end elsewhere than at n_cp or pass max_len;" if e & 1 else "",
                                " an index lies outside its pool or a row outside [0, n1)" if e & 2 else ""))


def lcs_ratio_pairs(pool1, pool2, pairs, out=None, err_flag=None):
    """pairs device int32 [n, 2] (string of pool1, string of pool2) -> (lcs int32 [n], ratio fp64 [n]) = (LCS length,
    Levenshtein.ratio = 2 lcs / (len1 + len2), 1.0 for two empty strings) (oea_lcs_ratio_pairs).  With err_flag given (device
    int32 [1], zeroed) the caller checks it (lcs_check); otherwise this call does, which waits for the device."""
    n = pairs.shape[0]
    dev = pool1.cp.device
    lcs, ratio = out if out is not None else (torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.float64, device=dev))
    flag = err_flag if err_flag is not None else torch.zeros(1, dtype=torch.int32, device=dev)
    max_len, ws = _lcs_workspace(pool1, pool2)
    check(lib().oea_lcs_ratio_pairs(*pool1._args(), *pool2._args(), max_len, _p(pairs), n, _p(lcs), _p(ratio), _p(ws), _p(flag), _stream()))
    if err_flag is None:
        lcs_check(flag)
    return lcs, ratio


def attr_sim_records_raw(pool1, pool2, idx1, idx2, threshold, cap, rows=None, out=None, err_flag=None):
    """One oea_attr_sim_records call, nothing read back -> (rec_col int32 [n_rows, cap], rec_val fp64 [n_rows, cap], rec_cnt int32
    [n_rows], overflow int32 [n_rows], err_flag)."""
    K, n1 = idx1.shape
    n2 = idx2.shape[1]
    dev = idx1.device
    n_rows = n1 if rows is None else rows.numel()
    if out is None:
        out = (torch.empty((n_rows, max(cap, 0)), dtype=torch.int32, device=dev), torch.empty((n_rows, max(cap, 0)), dtype=torch.float64, device=dev),
               torch.empty(n_rows, dtype=torch.int32, device=dev), torch.empty(n_rows, dtype=torch.int32, device=dev))
    flag = err_flag if err_flag is not None else torch.zeros(1, dtype=torch.int32, device=dev)
    max_len, ws = _lcs_workspace(pool1, pool2)
    check(lib().oea_attr_sim_records(*pool1._args(), *pool2._args(), max_len, K, _p(idx1), n1, _p(idx2), n2, float(threshold), _p(rows),
                                     n_rows, int(cap), _p(out[0]), _p(out[1]), _p(out[2]), _p(out[3]), _p(ws), _p(flag), _stream()))
    return out + (flag,)


def attr_sim_records(pool1, pool2, idx1, idx2, threshold, cap=16):
    """The records of every row of run_one_ea's walk (imuse.py:47-62) as a host CSR -> (ptr int64 [n1 + 1], col int32 [nnz], val fp64
    [nnz]): row i's records are the (j, s), j ascending, with s > threshold and s > every earlier s of the row, s the mean
    Levenshtein.ratio over the aligned attribute pairs both entities hold.  idx1 int32 [K, n1] / idx2 int32 [K, n2] on the device:
    value indices into the pools, -1 for none.  Rows that have more than `cap` records are run again with twice the capacity
    until none is left: no record is lost."""
    n1 = idx1.shape[1]
    counts = np.zeros(n1, np.int64)
    passes = []
    rows, rows_h = None, np.arange(n1)
    while rows_h.size:
        rec_col, rec_val, rec_cnt, overflow, flag = attr_sim_records_raw(pool1, pool2, idx1, idx2, threshold, cap, rows)
        lcs_check(flag)
        done = overflow.cpu().numpy() == 0
        cnt = rec_cnt.cpu().numpy().astype(np.int64)[done]
        counts[rows_h[done]] = cnt
        passes.append((rows_h[done], cnt, rec_col.cpu().numpy()[done], rec_val.cpu().numpy()[done]))
        rows_h = rows_h[~done]
        rows = to_ids(rows_h, idx1.device)
        cap *= 2
    ptr = np.zeros(n1 + 1, np.int64)
    np.cumsum(counts, out=ptr[1:])
    col, val = np.empty(ptr[-1], np.int32), np.empty(ptr[-1], np.float64)
    for r, cnt, c, v in passes:
        keep = np.arange(c.shape[1])[None, :] < cnt[:, None]
        at = (ptr[r][:, None] + np.arange(c.shape[1])[None, :])[keep]
        col[at], val[at] = c[keep], v[keep]
    return ptr, col, val


ATTR2VEC_VARS = ("embeds", "nce_weights", "nce_biases")
LOG_UNIFORM_STEPS_MAX_CLASSES = 8192


def log_uniform_sample_steps(n_classes, n_sampled, seed, step0, n_steps, thresholds, out=None):
    """The candidate sets of steps step0 .. step0 + n_steps in one launch (oea_log_uniform_sample_steps) -> (ids int32 [n_steps, S],
    num_tries int64 [n_steps], log Q fp32 [n_steps, S], status int32 [n_steps]): per step what LogUniformSampler.sample writes,
    without its host wait; status != 0 marks a step whose draw did not finish (check it once per epoch)."""
    dev = thresholds.device
    if out is None:
        out = (torch.zeros((n_steps, n_sampled), dtype=torch.int32, device=dev), torch.zeros(n_steps, dtype=torch.int64, device=dev),
               torch.zeros((n_steps, n_sampled), dtype=torch.float32, device=dev), torch.zeros(n_steps, dtype=torch.int32, device=dev))
    ids, tries, logq, status = out
    check(lib().oea_log_uniform_sample_steps(int(n_classes), int(n_sampled), int(seed) & (2 ** 64 - 1), int(step0) & (2 ** 64 - 1),
                                             int(n_steps), _p(thresholds), _p(ids), _p(tries), _p(logq), _p(status), _stream()))
    return out


def attr2vec_workspace(n_attr, ld, max_sampled, dev=None):
    """workspace of attr2vec_step / attr2vec_epoch for up to max_sampled candidates (zeroed once)"""
    n = lib().oea_attr2vec_workspace_bytes(int(n_attr), int(ld), int(max_sampled))
    if n == 0:
        raise OpenEAHipError("oea_attr2vec_workspace_bytes: n_attr=%d ld=%d max_sampled=%d" % (n_attr, ld, max_sampled))
    ws = torch.zeros(n, dtype=torch.uint8, device=dev or device())
    ws._shape = (int(n_attr), int(ld), int(max_sampled))
    return ws


def attr2vec_grads(workspace):
    """views of the three dense fp32 gradients a PHASE_GRAD call left in the workspace, in the order of ATTR2VEC_VARS"""
    n_attr, ld, max_s = workspace._shape
    ptrs = (C.c_void_p * 3)()
    check(lib().oea_attr2vec_grads(_p(workspace), n_attr, ld, max_s, ptrs))
    out = []
    for ptr, shape in zip(ptrs, ((n_attr, ld), (n_attr, ld), (n_attr,))):
        off = ptr - workspace.data_ptr()
        out.append(workspace[off:off + 4 * int(np.prod(shape))].view(torch.float32).view(shape))
    return out


def _attr2vec_vars(variables, accs):
    accs = accs or (None, None, None)
    for t in list(variables) + [a for a in accs if a is not None]:
        assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32
    v = _lib.Attr2VecVars(*[None if t is None else t.data_ptr() for pair in zip(variables, accs) for t in pair])
    v._keep = (variables, accs)
    return v


def attr2vec_step(variables, accs, dim, pairs, sampled, log_q, num_tries, lr, workspace, loss_accum, phase=PHASE_BOTH):
    """One Attr2Vec step in place (oea_attr2vec_step).  variables = (embeds [A, ld], nce_weights [A, ld], nce_biases [A]), accs their
    Adagrad accumulators; pairs int32 [B, 2] = (input, label); sampled / log_q [S] and num_tries (int64 [1]) from a sampler.  The
    batch mean is added to `loss_accum`."""
    n_attr, ld, max_s = workspace._shape
    assert variables[0].shape == (n_attr, ld) and pairs.dtype == torch.int32 and pairs.shape[1] == 2
    check(lib().oea_attr2vec_step(C.byref(_attr2vec_vars(variables, accs)), n_attr, dim, ld, _p(pairs), pairs.shape[0], _p(sampled),
                                  sampled.numel(), _p(log_q), _p(num_tries), float(lr), _p(workspace), max_s, _p(loss_accum),
                                  int(phase), _stream()))


def attr2vec_epoch(variables, accs, dim, pairs, batch, steps, seed, step0, thresholds, n_sampled, lr, workspace, loss_accum,
                   buffers=None):
    """`steps` Attr2Vec steps over the device list pairs [n_pairs, 2] in one call (oea_attr2vec_epoch): step s trains on
    pairs[sample_distinct(n_pairs, batch, seed, step0 + s)] with the candidates of log_uniform_sample_steps(seed, step0 + s).
    -> buffers (ids, num_tries, log_q, status, batch_idx) to pass back in; status is NOT read here."""
    n_attr, ld, max_s = workspace._shape
    dev = pairs.device
    if buffers is None:
        buffers = (torch.zeros((steps, n_sampled), dtype=torch.int32, device=dev), torch.zeros(steps, dtype=torch.int64, device=dev),
                   torch.zeros((steps, n_sampled), dtype=torch.float32, device=dev), torch.zeros(steps, dtype=torch.int32, device=dev),
                   torch.zeros(batch, dtype=torch.int32, device=dev))
    ids, tries, logq, status, idx = buffers
    assert ids.shape == (steps, n_sampled) and idx.numel() >= batch
    check(lib().oea_attr2vec_epoch(C.byref(_attr2vec_vars(variables, accs)), n_attr, dim, ld, _p(pairs), pairs.shape[0], int(batch),
                                   int(steps), int(seed) & (2 ** 64 - 1), int(step0) & (2 ** 64 - 1), _p(thresholds), int(n_sampled),
                                   _p(ids), _p(tries), _p(logq), _p(status), _p(idx), float(lr), _p(workspace), max_s, _p(loss_accum),
                                   _stream()))
    return buffers


# ---- ProjE ------------------------------------------------------------------------------------------------------
PROJE_MAX_DIM = 128
PROJE_VARS = ("ent_embeds", "rel_embeds", "entity_w", "entity_b", "input_bn_beta", "mlp_w", "mlp_bias", "output_bn_beta")


def log_uniform_thresholds(n_classes, dev=None):
    """T[c] = log(c + 2) / log(E + 1) in fp64, built on the host: the table oea_log_uniform_sample searches."""
    t = np.log(np.arange(2, int(n_classes) + 2, dtype=np.float64)) / np.log(np.float64(int(n_classes) + 1))
    return torch.from_numpy(t).to(dev or device())


class LogUniformSampler:
    """tf.nn.log_uniform_candidate_sampler(unique=True) on the device: sample(step) -> (ids int32 [S] in the order of first
    appearance, num_tries int64[1], log Q of the ids fp32 [S]); a pure function of (seed, step)."""

    def __init__(self, n_classes, n_sampled, seed, dev=None):
        dev = dev or device()
        self.n_classes, self.n_sampled, self.seed = int(n_classes), int(n_sampled), int(seed) & (2 ** 64 - 1)
        self.thresholds = log_uniform_thresholds(n_classes, dev) if n_classes >= 1 else None
        nbytes = lib().oea_log_uniform_workspace_bytes(self.n_classes, self.n_sampled)
        self.workspace = torch.zeros(max(nbytes, 1), dtype=torch.uint8, device=dev)
        self.ids = torch.zeros(max(self.n_sampled, 1), dtype=torch.int32, device=dev)
        self.num_tries = torch.zeros(1, dtype=torch.int64, device=dev)
        self.log_q = torch.zeros(max(self.n_sampled, 1), dtype=torch.float32, device=dev)

    def sample(self, step):
        check(lib().oea_log_uniform_sample(self.n_classes, self.n_sampled, self.seed, int(step), _p(self.thresholds), _p(self.ids),
                                           _p(self.num_tries), _p(self.log_q), _p(self.workspace), _stream()))
        return self.ids, self.num_tries, self.log_q


def proje_workspace(n_ent, n_rel, dim, ld, max_pos, max_sampled, dev=None):
    """workspace of proje_step for batches of up to max_pos positives and max_sampled candidates (zeroed once)"""
    n = lib().oea_proje_workspace_floats(int(n_ent), int(n_rel), int(dim), int(ld), int(max_pos), int(max_sampled))
    if n == 0:
        # the shape is refused: the accessor says why
        check(lib().oea_proje_grads(None, int(n_ent), int(n_rel), int(dim), int(ld), int(max_pos), int(max_sampled), None))
    ws = torch.zeros(n, dtype=torch.float32, device=dev or device())
    ws._proje_shape = (int(n_ent), int(n_rel), int(dim), int(ld), int(max_pos), int(max_sampled))
    return ws


def proje_grads(workspace):
    """the eight dense fp32 gradients a PHASE_GRAD call left in the workspace, as views (order: PROJE_VARS)"""
    n_ent, n_rel, dim, ld, max_pos, max_s = workspace._proje_shape
    ptrs = (C.c_void_p * 8)()
    check(lib().oea_proje_grads(_p(workspace), n_ent, n_rel, dim, ld, max_pos, max_s, ptrs))
    base = workspace.data_ptr()
    shapes = [(n_ent, ld), (n_rel, ld), (n_ent, ld), (n_ent,), (dim,), (dim,), (dim,), (dim,)]
    out = []
    for ptr, shp in zip(ptrs, shapes):
        off = (ptr - base) // 4
        out.append(workspace[off:off + int(np.prod(shp))].view(*shp))
    return out


def proje_step(variables, moments_m, moments_v, dim, pos, sampled, log_q, num_tries, t, lr, workspace, loss_accum,
               phase=PHASE_BOTH, check_ids=True):
    """One ProjE step in place (oea_proje_step).  variables / moments_m / moments_v: eight device fp32 tensors each in the order of
    PROJE_VARS (tables [n, ld], entity_b [n_ent], the four vectors [dim]); pos int32 [n, 3]; sampled, log_q, num_tries as
    LogUniformSampler.sample returned them.  check_ids: refuse ids outside the tables here (the kernels do not look)."""
    n_ent, n_rel, wdim, ld, max_pos, max_s = workspace._proje_shape
    ent, rel = variables[0], variables[1]
    assert len(variables) == len(moments_m) == len(moments_v) == 8
    assert ent.shape == (n_ent, ld) and rel.shape == (n_rel, ld) and variables[2].shape == (n_ent, ld) and wdim == dim
    assert variables[3].numel() == n_ent and all(x.numel() == dim for x in variables[4:])
    if check_ids and pos.numel():
        hi = pos.max(dim=0).values.tolist()
        lo = int(pos.min())
        if lo < 0 or hi[0] >= n_ent or hi[1] >= n_rel or hi[2] >= n_ent or int(sampled.max()) >= n_ent or int(sampled.min()) < 0:
            raise OpenEAHipError("proje_step: an id lies outside its table (entities %d, relations %d)" % (n_ent, n_rel))
    v = _lib.ProjEVars()
    for i in range(8):
        v.p[i], v.m[i], v.v[i] = variables[i].data_ptr(), moments_m[i].data_ptr(), moments_v[i].data_ptr()
    for x in list(variables) + list(moments_m) + list(moments_v):
        assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float32
    check(lib().oea_proje_step(C.byref(v), n_ent, n_rel, dim, ld, _p(pos), pos.shape[0], _p(sampled), _p(log_q), sampled.numel(),
                               _p(num_tries), int(t), float(lr), _p(workspace), max_pos, max_s, _p(loss_accum), int(phase),
                               _stream()))


# ---- ConvE -------------------------------------------------------------------------------------------------------
CONVE_MAX_FILTERS = 64
CONVE_VARS = ("ent_embeds", "rel_embeds", "entity_w", "entity_b", "gamma1", "beta1", "kern", "cbias", "gamma2", "beta2", "fcW", "fcb",
              "gamma3", "beta3")


def dim_factorization(d):
    """conve.py:10-18 without the print: (x, y), x the largest divisor of d below sqrt(d) + 1, y = d // x"""
    half = int(math.sqrt(d)) + 1
    while d % half > 0:
        half -= 1
    return half, d // half


def _conve_shapes(n_ent, n_rel, dim, ld, filters):
    y = dim_factorization(dim)[1]
    return [(n_ent, ld), (n_rel, ld), (n_ent, ld), (n_ent,), (y,), (y,), (9 * filters,), (filters,), (filters,), (filters,),
            (2 * dim * filters, ld), (dim,), (dim,), (dim,)]


def conve_workspace(n_ent, n_rel, dim, ld, filters, max_pos, max_sampled, dev=None):
    """workspace of conve_step for batches of up to max_pos positives and max_sampled candidates (zeroed once)"""
    shape = (int(n_ent), int(n_rel), int(dim), int(ld), int(filters), int(max_pos), int(max_sampled))
    n = lib().oea_conve_workspace_floats(*shape)
    if n == 0:
        # the shape is refused: the accessor says why
        check(lib().oea_conve_grads(None, *shape, None))
    ws = torch.zeros(n, dtype=torch.float32, device=dev or device())
    ws._conve_shape = shape
    return ws


def conve_grads(workspace):
    """the fourteen dense fp32 gradients a PHASE_GRAD call left in the workspace, as views (order: CONVE_VARS; kern as [9 F],
    tap-major, which is [3, 3, 1, F] flattened)"""
    n_ent, n_rel, dim, ld, filters, max_pos, max_s = workspace._conve_shape
    ptrs = (C.c_void_p * 14)()
    check(lib().oea_conve_grads(_p(workspace), n_ent, n_rel, dim, ld, filters, max_pos, max_s, ptrs))
    base = workspace.data_ptr()
    out = []
    for ptr, shp in zip(ptrs, _conve_shapes(n_ent, n_rel, dim, ld, filters)):
        off = (ptr - base) // 4
        out.append(workspace[off:off + int(np.prod(shp))].view(*shp))
    return out


def conve_step(variables, moments_m, moments_v, dim, filters, keep_prob, seed, pos, sampled, log_q, num_tries, mask_step, t, lr,
               workspace, loss_accum, phase=PHASE_BOTH, check_ids=True):
    """One ConvE step in place (oea_conve_step).  variables / moments_m / moments_v: fourteen device fp32 tensors each in the order
    of CONVE_VARS (tables [n, ld], fcW [2 dim F, ld], kern [9 F] or [3, 3, 1, F]); pos int32 [n, 3]; sampled, log_q, num_tries as
    LogUniformSampler.sample returned them; (seed, mask_step) select the dropout masks.  check_ids: refuse ids outside the tables
    here (the kernels do not look)."""
    n_ent, n_rel, wdim, ld, wf, max_pos, max_s = workspace._conve_shape
    assert len(variables) == len(moments_m) == len(moments_v) == 14 and wdim == dim and wf == filters
    if dim <= PROJE_MAX_DIM and 1 <= filters <= CONVE_MAX_FILTERS:
        for x, shp in zip(variables, _conve_shapes(n_ent, n_rel, dim, ld, filters)):
            assert x.numel() == int(np.prod(shp)) and (len(shp) == 1 or tuple(x.shape) == shp), (tuple(x.shape), shp)
    if check_ids and pos.numel():
        hi = pos.max(dim=0).values.tolist()
        lo = int(pos.min())
        if lo < 0 or hi[0] >= n_ent or hi[1] >= n_rel or hi[2] >= n_ent or int(sampled.max()) >= n_ent or int(sampled.min()) < 0:
            raise OpenEAHipError("conve_step: an id lies outside its table (entities %d, relations %d)" % (n_ent, n_rel))
    v = _lib.ConvEVars()
    for i in range(14):
        v.p[i], v.m[i], v.v[i] = variables[i].data_ptr(), moments_m[i].data_ptr(), moments_v[i].data_ptr()
    for x in list(variables) + list(moments_m) + list(moments_v):
        assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float32
    cfg = _lib.ConvECfg(int(filters), float(keep_prob), int(seed) & (2 ** 64 - 1))
    check(lib().oea_conve_step(C.byref(v), C.byref(cfg), n_ent, n_rel, dim, ld, _p(pos), pos.shape[0], _p(sampled), _p(log_q),
                               sampled.numel(), _p(num_tries), int(mask_step) & (2 ** 64 - 1), int(t), float(lr), _p(workspace), max_pos,
                               max_s, _p(loss_accum), int(phase), _stream()))


# ---- IPTransE ---------------------------------------------------------------------------------------------------
PATH_MAX_REL = 2048


def path_workspace(n_rel, ld, dev=None):
    """scratch of oea_path_grad / oea_ptranse_step for a relation table of n_rel rows (zeroed once; the calls leave its zero part
    zeroed) + the int32 error flag of the device-side id check: -> (workspace, err_flag)"""
    dev = dev or device()
    nbytes = lib().oea_path_workspace_bytes(int(n_rel), int(ld))
    return torch.zeros(max(nbytes, 1), dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)


def path_check(err_flag):
    """raise if the device-side id check of the path steps found an id outside the relation table (one sync); clears the flag"""
    code = int(err_flag.item())
    if code != 0:
        err_flag.zero_()
        raise OpenEAHipError("libopenea_hip error %d: a path id outside [0, n_rel) (err_flag %d): the path batch was left out"
                             % (-1, code))


def path_grad(rel, dim, paths, neg_rel, weight, margin, path_parm, rel_l2_norm, workspace, n_ent, path_ws, loss_accum, check_ids=True):
    """the path half of IPTransE's step (oea_path_grad): adds its gradient w.r.t. the normalised relation rows into the step
    workspace's scratch and path_parm * path loss to `loss_accum`; follow with triple_step(..., phase=PHASE_APPLY).  paths device
    int32 [n, 3] = (r_x, r_y, r), neg_rel int32 [n], weight fp32 [n]; path_ws = path_workspace(...).  check_ids: read the id
    check's flag (one sync) and raise on an id outside the table."""
    ws, err = path_ws
    n = paths.shape[0]
    assert neg_rel.numel() == n and weight.numel() == n
    check(lib().oea_path_grad(_p(rel), rel.shape[0], dim, rel.shape[1], _p(paths), _p(neg_rel), _p(weight), n, float(margin),
                              float(path_parm), int(bool(rel_l2_norm)), _p(workspace), int(n_ent), _p(ws), _p(loss_accum), _p(err),
                              _stream()))
    if check_ids and n:
        path_check(err)


def ptranse_step(ent, ent_acc, rel, rel_acc, dim, pos, neg, paths, neg_rel, weight, path_parm, cfg, workspace, path_ws, loss_accum,
                 check_ids=True):
    """One IPTransE optimiser step in place (oea_ptranse_step): margin pairs (pos i, neg i) + the path batch, one apply phase on
    the summed gradient; `loss_accum` += triple loss + path_parm * path loss.  paths may be None / empty (plain margin step)."""
    ws, err = path_ws
    n_p = 0 if paths is None else paths.shape[0]
    n_neg = 0 if neg is None else neg.shape[0]
    check(lib().oea_ptranse_step(_p(ent), _p(ent_acc), ent.shape[0], _p(rel), _p(rel_acc), rel.shape[0], dim, ent.shape[1],
                                 _p(pos), pos.shape[0], _p(neg), n_neg, _p(paths) if n_p else None, _p(neg_rel) if n_p else None,
                                 _p(weight) if n_p else None, n_p, float(path_parm), C.byref(cfg), _p(workspace), _p(ws),
                                 _p(loss_accum), _p(err), _stream()))
    if check_ids and n_p:
        path_check(err)


def path_sample_dims(n1, n2, steps):
    """-> (P, num1) of a step's path batch (iptranse.py:77, 245)"""
    P = (n1 + n2) // steps
    return P, (int(n1 / (n1 + n2) * P) if P else 0)


def path_sample_epoch(paths1, weight1, paths2, weight2, rels1, rels2, steps, seed, epoch, out=None):
    """the path batches of an epoch in one launch (oea_path_sample_epoch) -> (paths [steps, P, 3] int32, neg_rel [steps, P] int32,
    weight [steps, P] fp32) on the device; paths* int32 [n, 3], weight* fp32 [n], rels* int32 relation lists."""
    n1, n2 = paths1.shape[0], paths2.shape[0]
    P, _ = path_sample_dims(n1, n2, steps) if n1 + n2 else (0, 0)
    dev = paths1.device
    if out is None or out[0].shape != (steps, P, 3):
        out = (torch.empty((steps, P, 3), dtype=torch.int32, device=dev), torch.empty((steps, P), dtype=torch.int32, device=dev),
               torch.empty((steps, P), dtype=torch.float32, device=dev))
    check(lib().oea_path_sample_epoch(_p(paths1), _p(weight1), n1, _p(paths2), _p(weight2), n2, _p(rels1), rels1.numel(), _p(rels2),
                                      rels2.numel(), int(steps), int(seed), int(epoch), _p(out[0]), _p(out[1]), _p(out[2]),
                                      _stream()))
    return out


def ptranse_epoch(ent, ent_acc, rel, rel_acc, dim, pos_all, offsets, neg_all, path_batches, path_parm, cfg, workspace, path_ws,
                  loss_accum, check_ids=True):
    """every step of an IPTransE epoch with one call (oea_ptranse_epoch): offsets host int64 [steps + 1] into pos_all / neg_all
    (one negative per positive, already drawn), path_batches = path_sample_epoch's three buffers (or None: plain margin steps)."""
    ws, err = path_ws
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    steps = len(offsets) - 1
    P = 0 if path_batches is None else int(path_batches[0].shape[1])
    if P:
        assert path_batches[0].shape[0] == steps
    pb = path_batches if P else (None, None, None)
    check(lib().oea_ptranse_epoch(_p(ent), _p(ent_acc), ent.shape[0], _p(rel), _p(rel_acc), rel.shape[0], dim, ent.shape[1],
                                  _p(pos_all), offsets.ctypes.data_as(C.c_void_p), steps, _p(neg_all), _p(pb[0]), _p(pb[1]),
                                  _p(pb[2]), P, float(path_parm), C.byref(cfg), _p(workspace), _p(ws), _p(loss_accum), _p(err),
                                  _stream()))
    if check_ids and P:
        path_check(err)


def weighted_pair_step(ent, ent_acc, rel, rel_acc, dim, pos, neg, weight, cfg, workspace, loss_accum):
    """One step of IPTransE's alignment loss in place (oea_weighted_pair_step): sum_i weight[i] relu(pos_i + margin - neg_i) over
    the pairs (pos i, neg i), int32 [n, 3] each, weight fp32 [n]."""
    n = pos.shape[0]
    assert neg.shape[0] == n and weight.numel() == n
    check(lib().oea_weighted_pair_step(_p(ent), _p(ent_acc), ent.shape[0], _p(rel), _p(rel_acc), rel.shape[0], dim, ent.shape[1],
                                       _p(pos), _p(neg), _p(weight), n, C.byref(cfg), _p(workspace), _p(loss_accum), _stream()))


def part_rows_per_rank(n_ent, world):
    return int(lib().oea_part_rows_per_rank(int(n_ent), int(world)))


def part_pack(workspace, n_ent, n_rel, ld, world, send, rel_x):
    check(lib().oea_part_pack(_p(workspace), n_ent, n_rel, ld, world, _p(send), _p(rel_x), _stream()))


def part_apply(ent, acc_own, rel, rel_acc, world, rank, own, rel_x, upd, cfg, workspace, n_items, loss_accum):
    check(lib().oea_part_apply(_p(ent), _p(acc_own), ent.shape[0], _p(rel), _p(rel_acc), rel.shape[0], ent.shape[1], world, rank,
                               _p(own), _p(rel_x), _p(upd), C.byref(cfg), _p(workspace), int(n_items), _p(loss_accum), _stream()))


def part_unpack(ent, world, rank, all_rows):
    check(lib().oea_part_unpack(_p(ent), ent.shape[0], ent.shape[1], world, rank, _p(all_rows), _stream()))


def step_exchange_view(workspace, n_ent, n_rel, ld):
    """view (fp32, or int64 in the deterministic build) of the workspace region (gradient scratch + touched flags) that
    data-parallel ranks sum with one all-reduce."""
    n = lib().oea_step_exchange_floats(n_ent, n_rel, ld)
    dt = scratch_dtype()
    return workspace[: dt.itemsize * n].view(dt)


def step_entity_flags(workspace, n_ent, n_rel, ld):
    """the entity rows' touched flags inside the step workspace (a view; scratch element type): nonzero = the row received gradient
    through the atomic scratch in the GRAD phase that just ran"""
    eg, et = C.c_void_p(), C.c_void_p()
    check(lib().oea_step_entity_scratch(_p(workspace), int(n_ent), int(n_rel), int(ld), C.byref(eg), C.byref(et)))
    dt = scratch_dtype()
    off = et.value - workspace.data_ptr()
    return workspace[off: off + dt.itemsize * int(n_ent)].view(dt)


def step_normal_views(workspace, n_ent, n_rel, ld):
    """TransH under the entity-id partition: fp32 views of the normal-vector gradient scratch [n_rel * ld] and its touched
    flags [n_rel] inside the step workspace (summed over the ranks after the GRAD phase, include/openea_hip.h)."""
    g_off, t_off = C.c_int64(0), C.c_int64(0)
    check(lib().oea_step_normal_scratch(int(n_ent), int(n_rel), int(ld), C.byref(g_off), C.byref(t_off)))
    dt = scratch_dtype()
    grad = workspace[g_off.value: g_off.value + dt.itemsize * n_rel * ld].view(dt)
    touched = workspace[t_off.value: t_off.value + dt.itemsize * n_rel].view(dt)
    return grad, touched


def step_apply_normals(n_ent, n_rel, ld, cfg, workspace):
    check(lib().oea_step_apply_normals(int(n_ent), int(n_rel), int(ld), C.byref(cfg), _p(workspace), _stream()))


def profile_begin(stride=1):
    check(lib().oea_profile_begin(int(stride)))


def profile_end(group=4):
    ms = (C.c_double * (group - 1))()
    n = C.c_int32(0)
    check(lib().oea_profile_end(group, ms, C.byref(n)))
    return [float(x) for x in ms], int(n.value)


# -------------------------------------------------------------------------------------------
# sampler
# -------------------------------------------------------------------------------------------


def tripleset_build(triples):
    """device int32 [n,3] -> device uint64 table (viewed as int64)."""
    n = triples.shape[0]
    if n:   # key layout (csrc/common.h:pack_triple): head 24 | relation 16 | tail 24 bits -- larger ids would alias
        mx = triples.max(dim=0).values.cpu()
        if int(mx[0]) >= 1 << 24 or int(mx[2]) >= 1 << 24 or int(mx[1]) >= 1 << 16 or int(triples.min().item()) < 0:
            raise OpenEAHipError("triple ids out of range for the packed membership keys "
                                 "(entity ids < 16,777,216, relation ids < 65,536)")
    cap = lib().oea_tripleset_capacity(n)
    table = torch.empty(cap, dtype=torch.int64, device=triples.device)
    check(lib().oea_tripleset_build(_p(triples), n, _p(table), cap, _stream()))
    return table


def sample_negatives(pos, k, table, entity_list, ent_pos=None, nbr=None, seed=0, step=0,
                     pos_offset=0, max_try=10, out=None, err_flag=None):
    n_pos = pos.shape[0]
    if out is None:
        out = torch.empty((n_pos * k, 3), dtype=torch.int32, device=pos.device)
    if err_flag is None:
        err_flag = torch.zeros(1, dtype=torch.int32, device=pos.device)
    nbr_k = 0 if nbr is None else nbr.shape[1]
    check(lib().oea_sample_negatives(_p(pos), n_pos, k, _p(table), table.numel(), _p(entity_list),
                                     entity_list.numel(), _p(ent_pos), _p(nbr), nbr_k, int(seed),
                                     int(step), int(pos_offset), int(max_try), _p(out), _p(err_flag),
                                     _stream()))
    return out, err_flag


def sample_negatives_replay(pos, k, table, entity_list, replay, ent_pos=None, nbr=None, max_try=10):
    """the sampler kernel fed from a recorded run of the reference (oea_sample_negatives_replay): replay int32
    [n_pos, max_try, 1 + k] = per round the side bit and the candidate-list positions random.sample returned"""
    n_pos = pos.shape[0]
    out = torch.zeros((n_pos * k, 3), dtype=torch.int32, device=pos.device)
    err_flag = torch.zeros(1, dtype=torch.int32, device=pos.device)
    nbr_k = 0 if nbr is None else nbr.shape[1]
    assert tuple(replay.shape) == (n_pos, max_try, 1 + k) and replay.dtype == torch.int32 and replay.is_contiguous()
    check(lib().oea_sample_negatives_replay(_p(pos), n_pos, k, _p(table), table.numel(), _p(entity_list), entity_list.numel(),
                                            _p(ent_pos), _p(nbr), nbr_k, int(max_try), _p(replay), _p(out), _p(err_flag), _stream()))
    return out, err_flag


def tripleset_filter(triples, capacity):
    """the "certainly absent" bit array over the triples of a membership table of `capacity` slots (oea_tripleset_filter_build)
    -> device int32 [capacity / 4] (8 x capacity bits)"""
    bits = int(lib().oea_tripleset_filter_bits(int(capacity)))
    filt = torch.empty(bits // 32, dtype=torch.int32, device=triples.device)
    check(lib().oea_tripleset_filter_build(_p(triples), triples.shape[0], _p(filt), bits, _stream()))
    return filt


def sampler_side(table, entity_list, ent_pos, nbr, filt=None):
    """pack one KG's sampler state for sample_negatives_pair (keeps the tensors alive)."""
    side = _lib.SamplerSide(table.data_ptr(), table.numel(), entity_list.data_ptr(),
                            ent_pos.data_ptr() if ent_pos is not None else None,
                            nbr.data_ptr() if nbr is not None else None, entity_list.numel(),
                            0 if nbr is None else nbr.shape[1],
                            filt.data_ptr() if filt is not None else None, 0 if filt is None else 32 * filt.numel())
    side._keep = (table, entity_list, ent_pos, nbr, filt)
    return side


def sample_negatives_pair(pos, n_split, k, side0, side1, seed, step, pos_offset, out, err_flag, max_try=10):
    """one launch for pos_batch1 + pos_batch2 (batch.py:36-45): rows [0, n_split) against side0."""
    check(lib().oea_sample_negatives_pair(_p(pos), pos.shape[0], int(n_split), k, C.byref(side0), C.byref(side1),
                                          int(seed), int(step), int(pos_offset), int(max_try), _p(out), _p(err_flag),
                                          _stream()))
    return out


def sample_negatives_epoch(pos_all, offsets_dev, splits_dev, steps, k, side0, side1, seed, step_base, out, err_flag, max_try=10):
    """negatives of every batch of an epoch in one launch (on the CURRENT torch stream)."""
    check(lib().oea_sample_negatives_epoch(_p(pos_all), pos_all.shape[0], _p(offsets_dev), _p(splits_dev), int(steps), int(k),
                                           C.byref(side0), C.byref(side1), int(seed), int(step_base), int(max_try), _p(out),
                                           _p(err_flag), _stream()))
    return out


def _epoch(ent, ent_acc, rel, rel_acc, dim, pos_all, offsets, splits, k, side0, side1, seed, step_base, neg_buf, err_flag, cfg,
           workspace, loss_accum, offsets_dev, splits_dev, step_range):
    """-> (_lib.Epoch, lo, hi): the descriptor the three epoch calls share (oea_epoch) and the step range, default the whole epoch"""
    offsets, splits = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(splits, np.int64)   # what the C side reads
    steps = len(splits)
    e = _lib.Epoch(_p(ent), _p(ent_acc), ent.shape[0], _p(rel), _p(rel_acc), rel.shape[0], dim, ent.shape[1],
                   _p(pos_all), offsets.ctypes.data, splits.ctypes.data, steps, _p(offsets_dev), _p(splits_dev),
                   int(k), C.pointer(side0) if side0 is not None else None, C.pointer(side1) if side1 is not None else None,
                   int(seed), int(step_base), _p(neg_buf), _p(err_flag), C.pointer(cfg), _p(workspace), _p(loss_accum))
    e._keep = (offsets, splits)
    lo, hi = (0, steps) if step_range is None else step_range
    return e, int(lo), int(hi)


def triple_epoch(ent, ent_acc, rel, rel_acc, dim, pos_all, offsets, splits, k, side0, side1, seed, step_base,
                 neg_buf, err_flag, cfg, workspace, loss_accum, offsets_dev=None, splits_dev=None, step_range=None, shard=(0, 1),
                 plan=None):
    """Enqueue every step of an epoch (or steps [lo, hi) of it: step_range) with one call (offsets / splits: host int64
    numpy arrays; their device copies enable sampling the whole epoch ahead in one launch -- neg_buf then covers the
    epoch).  step_base: Philox step of the epoch's step 0.  shard = (rank, world): this rank's contiguous share of every
    batch, trained on the local tables (dp_exchange = 'epoch').  plan = (buffer, built): the gathered-sum plan of the epoch
    (step_plan_buffer / step_plan_build; include/openea_hip.h), for shard (0, 1) only."""
    e, lo, hi = _epoch(ent, ent_acc, rel, rel_acc, dim, pos_all, offsets, splits, k, side0, side1, seed, step_base, neg_buf, err_flag,
                       cfg, workspace, loss_accum, offsets_dev, splits_dev, step_range)
    buf, built = plan if plan is not None else (None, False)
    check(lib().oea_triple_epoch_range(C.byref(e), lo, hi, int(shard[0]), int(shard[1]), _p(buf), buf.numel() if buf is not None else 0,
                                       int(bool(built)), _stream()))


def epoch_layout(triples, n1, n2, slot, seed, epoch, dall, workspace=None):
    """an epoch's shuffle of both triple lists + the batch layout gather (oea_epoch_layout) on the current stream -> workspace"""
    n = int(n1) + int(n2)
    if workspace is None:
        workspace = torch.empty(lib().oea_epoch_layout_bytes(n), dtype=torch.uint8, device=triples.device)
    check(lib().oea_epoch_layout(_p(triples), int(n1), int(n2), _p(slot), slot.numel(), int(seed) & 0xFFFFFFFFFFFFFFFF, int(epoch) & 0xFFFFFFFF,
                                 _p(dall), _p(workspace), workspace.numel(), _stream()))
    return workspace


def step_plan_supported(cfg, n_ent, n_rel, ld, k):
    """would an epoch under cfg run on the gathered-sum plan (oea_step_plan_supported)?"""
    return bool(lib().oea_step_plan_supported(C.byref(cfg), int(n_ent), int(n_rel), int(ld), int(k)))


def step_plan_buffer(n_total, steps, max_batch, n_ent, ld, dev=None):
    """workspace of one epoch's plan (oea_step_plan_bytes)"""
    nbytes = lib().oea_step_plan_bytes(int(n_total), int(steps), int(max_batch), int(n_ent), int(ld))
    return torch.empty(nbytes, dtype=torch.uint8, device=dev or device())


def step_plan_build(pos_all, neg_all, k, offsets_dev, n_total, steps, max_batch, n_ent, ld, plan):
    """sort the epoch's (step, row) references on the current stream (oea_step_plan_build): no allocation, no host read"""
    check(lib().oea_step_plan_build(_p(pos_all), _p(neg_all), int(k), _p(offsets_dev), int(n_total), int(steps), int(max_batch),
                                    int(n_ent), int(ld), _p(plan), plan.numel(), _stream()))


def step_plan_arrays(plan, n_total, steps, max_batch, n_ent, ld):
    """host copies of a built plan (tests): dict(vals uint32 [2 n_total], ukeys uint64 [n_unique], uoff uint32 [n_unique + 1],
    step_first int32 [steps + 1], row_bits, pflags uint32 [n_total])"""
    off = (C.c_int64 * 9)()
    check(lib().oea_step_plan_offsets(int(n_total), int(steps), int(max_batch), int(n_ent), int(ld), C.cast(off, C.c_void_p)))
    raw = plan.cpu().numpy()
    m = 2 * int(n_total)
    nu = int(raw[off[3]: off[3] + 4].view(np.int32)[0])
    return dict(vals=raw[off[0]: off[0] + 4 * m].view(np.uint32).copy(), ukeys=raw[off[1]: off[1] + 8 * nu].view(np.uint64).copy(),
                uoff=raw[off[2]: off[2] + 4 * (nu + 1)].view(np.uint32).copy(),
                step_first=raw[off[4]: off[4] + 4 * (steps + 1)].view(np.int32).copy(), row_bits=int(off[6]), n_unique=nu,
                pflags=raw[off[8]: off[8] + 4 * int(n_total)].view(np.uint32).copy())


def step_plan_rel_order(plan, n_total, steps, max_batch, n_ent, ld):
    """host copy of a built plan's rel_order (tests): uint32 [n_total], per step the batch-local indices of its positives in stable
    ascending order of relation id (oea_step_plan_rel_order_offset)"""
    off = C.c_int64(0)
    check(lib().oea_step_plan_rel_order_offset(int(n_total), int(steps), int(max_batch), int(n_ent), int(ld), C.cast(C.byref(off), C.c_void_p)))
    n = int(n_total)
    return plan[off.value: off.value + 4 * n].cpu().numpy().view(np.uint32).copy()


def step_plan_stats(plan, n_total, steps, max_batch, n_ent, ld):
    """what a built plan looks like (bench detail / experiments): positives outside the rule, references to hub rows, rows and
    entries per step"""
    a = step_plan_arrays(plan, n_total, steps, max_batch, n_ent, ld)
    last = int(a["step_first"][steps])                       # distinct keys of real steps
    cnt = np.diff(a["uoff"].astype(np.int64))[:last]
    listed = int(a["uoff"][last])                            # references of positives inside the rule
    hub = cnt > 8
    return dict(positives=int(n_total), outside_rule=int(n_total - listed // 2), rows_per_step=float(last) / max(steps, 1),
                refs_per_row_mean=float(cnt.mean()) if last else 0.0, refs_per_row_max=int(cnt.max()) if last else 0,
                hub_rows_per_step=float(hub.sum()) / max(steps, 1), refs_to_hub_rows=int(cnt[hub].sum()),
                refs_listed=listed)


def comm_single_or_none():
    """a one-rank communicator of the C ABI (tests): (handle, destroy)"""
    uid = (C.c_char * 128)()
    check(lib().oea_comm_unique_id(uid))
    comm = C.c_void_p()
    check(lib().oea_comm_init(uid, 0, 1, C.byref(comm)))
    return comm


def part_buffers(n_ent, n_rel, ld, world, dev, adagrad=True):
    """the exchange buffers of the partitioned step (include/openea_hip.h) + the optimiser state of the owned rows"""
    rpr = lib().oea_part_rows_per_rank(int(n_ent), int(world))
    chunk = rpr * (ld + 1)
    f = dict(dtype=torch.float32, device=dev)
    g = dict(dtype=scratch_dtype(), device=dev)         # the gradients travel in the scratch's own type
    return dict(rpr=rpr, chunk=chunk, send=torch.empty(world * chunk, **g), own=torch.empty(chunk, **g),
                rel_x=torch.empty(n_rel * (ld + 1), **g), upd=torch.empty((rpr, ld), **f), all=torch.empty((world, rpr, ld), **f),
                acc_own=torch.full((rpr, ld), 0.1, **f) if adagrad else None)


def triple_epoch_comm(comm, ent, acc_own, rel, rel_acc, dim, pos_all, offsets, splits, k, side0, side1, seed, step_base, neg_buf,
                      err_flag, cfg, workspace, loss_accum, offsets_dev, splits_dev, bufs, step_range=None):
    """steps [lo, hi) of a data-parallel epoch under the entity-id partition from ONE C call over the C ABI's communicator
    (oea_triple_epoch_range_comm); bufs = part_buffers(...)."""
    e, lo, hi = _epoch(ent, acc_own, rel, rel_acc, dim, pos_all, offsets, splits, k, side0, side1, seed, step_base, neg_buf, err_flag,
                       cfg, workspace, loss_accum, offsets_dev, splits_dev, step_range)
    check(lib().oea_triple_epoch_range_comm(comm, C.byref(e), lo, hi, _p(bufs['send']), _p(bufs['own']), _p(bufs['rel_x']),
                                            _p(bufs['upd']), _p(bufs['all']), _stream()))


def halo_buffers(n_ent, ld, world, steps, max_batch, k, dev):
    """workspace + the two exchange buffers of the boundary-row exchange (oea_triple_epoch_range_halo)"""
    wsb = lib().oea_halo_workspace_bytes(int(n_ent), int(world), int(steps), int(max_batch), int(k))
    xb = lib().oea_halo_buffer_bytes(int(n_ent), int(world), int(max_batch), int(k), int(ld))
    u8 = dict(dtype=torch.uint8, device=dev)
    return dict(ws=torch.empty(wsb, **u8), a=torch.empty(xb, **u8), b=torch.empty(xb, **u8), key=(int(steps), int(max_batch), int(k)))


def halo_plan(pos_all, neg_all, k, offsets, n_ent, world, step_range=None, with_lists=True):
    """which rows every rank's share of every step refers to, per owner (oea_halo_plan) -> (counts int32 [steps, world, world],
    lists int32 [steps, world, cap] or None): what sizes the messages of the boundary-row exchange"""
    offsets = np.ascontiguousarray(offsets, np.int64)      # ONE array for the host pointer and the device copy
    steps = len(offsets) - 1
    lo, hi = (0, steps) if step_range is None else step_range
    max_batch = int(np.diff(offsets).max()) if steps else 0
    dev = pos_all.device
    ws = torch.empty(lib().oea_halo_workspace_bytes(int(n_ent), int(world), hi - lo, max_batch, int(k)), dtype=torch.uint8, device=dev)
    off_dev = torch.from_numpy(offsets).to(dev)
    counts = np.zeros((hi - lo, world, world), np.int32)
    cap = C.c_int64(0)
    check(lib().oea_halo_plan(_p(pos_all), _p(neg_all), int(k), offsets.ctypes.data_as(C.c_void_p), _p(off_dev), steps, int(lo), int(hi),
                              int(n_ent), int(world), _p(ws), ws.numel(), counts.ctypes.data_as(C.c_void_p), None, C.byref(cap), _stream()))
    lists = None
    if with_lists:
        lists = np.zeros((hi - lo, world, int(cap.value)), np.int32)
        check(lib().oea_halo_plan(_p(pos_all), _p(neg_all), int(k), offsets.ctypes.data_as(C.c_void_p), _p(off_dev), steps, int(lo), int(hi),
                                  int(n_ent), int(world), _p(ws), ws.numel(), counts.ctypes.data_as(C.c_void_p),
                                  lists.ctypes.data_as(C.c_void_p), C.byref(cap), _stream()))
    return counts, lists


def triple_epoch_halo(comm, ent, acc_own, rel, rel_acc, dim, pos_all, offsets, splits, k, side0, side1, seed, step_base, neg_buf,
                      err_flag, cfg, workspace, loss_accum, offsets_dev, splits_dev, bufs, halo, step_range=None):
    """triple_epoch_comm with the boundary-row exchange (oea_triple_epoch_range_halo); bufs = part_buffers(...), halo =
    halo_buffers(...) -> (bytes pushed, bytes pulled, largest rows sent in a step, steps) of this rank"""
    e, lo, hi = _epoch(ent, acc_own, rel, rel_acc, dim, pos_all, offsets, splits, k, side0, side1, seed, step_base, neg_buf, err_flag,
                       cfg, workspace, loss_accum, offsets_dev, splits_dev, step_range)
    stats = (C.c_int64 * 4)()
    check(lib().oea_triple_epoch_range_halo(comm, C.byref(e), lo, hi, _p(halo['ws']), halo['ws'].numel(), _p(halo['a']), _p(halo['b']),
                                            halo['a'].numel(), _p(bufs['rel_x']), _p(bufs['upd']), _p(bufs['all']),
                                            C.cast(stats, C.c_void_p), _stream()))
    return tuple(int(x) for x in stats)


def sample_link_negatives(n_pos, k, pos_links=None, ents1=None, ents2=None, nbr1=None, row1=None, nbr2=None, row2=None,
                          exclude=None, seed=0, step=0, scratch=None):
    """AliNet.generate_input_batch negatives on the device -> (pairs int32 [m, 2], valid fp32 [m]).
    uniform: ents1 / ents2 (device int32 lists); truncated: pos_links [n_pos, 2] + nbr1/nbr2 [rows, nbr_k] + row maps.
    exclude: tripleset over (e1, 0, e2) (tripleset_build) or None."""
    truncated = nbr1 is not None
    m = (2 if truncated else 1) * k * n_pos
    dev = (nbr1 if truncated else ents1).device
    pairs = torch.empty((m, 2), dtype=torch.int32, device=dev)
    valid = torch.empty(m, dtype=torch.float32, device=dev)
    cap = 2
    while cap < 2 * max(m, 1):
        cap *= 2
    if scratch is None or scratch[0].numel() < cap:
        scratch = (torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(cap, dtype=torch.int32, device=dev))
    check(lib().oea_sample_link_negatives(_p(pos_links), n_pos, k, _p(ents1), 0 if ents1 is None else ents1.numel(),
                                          _p(ents2), 0 if ents2 is None else ents2.numel(), _p(nbr1), _p(row1), _p(nbr2),
                                          _p(row2), nbr1.shape[1] if truncated else 0, _p(exclude),
                                          0 if exclude is None else exclude.numel(), int(seed), int(step), _p(pairs),
                                          _p(valid), _p(scratch[0]), _p(scratch[1]), cap, _stream()))
    return pairs, valid, scratch


def greedy_matching(left, right, weight):
    """HOST numpy arrays -> bool mask of the edges kept by the weight-descending one-to-one selection."""
    left = np.ascontiguousarray(left, np.int32)
    right = np.ascontiguousarray(right, np.int32)
    weight = np.ascontiguousarray(weight, np.float32)
    sel = np.zeros(len(left), np.uint8)
    check(_lib.load(require_device=False).oea_greedy_matching(left.ctypes.data_as(C.c_void_p), right.ctypes.data_as(C.c_void_p),
                                                              weight.ctypes.data_as(C.c_void_p), len(left),
                                                              sel.ctypes.data_as(C.c_void_p)))
    return sel.astype(bool)


def pair_dots(e1, e2, dim, ii, jj):
    """device: out[i] = <e1[ii[i]], e2[jj[i]]>."""
    out = torch.empty(ii.numel(), dtype=torch.float32, device=e1.device)
    check(lib().oea_pair_dots(_p(e1), e1.shape[1], _p(e2), e2.shape[1], dim, _p(ii), _p(jj), ii.numel(), _p(out), _stream()))
    return out


# -------------------------------------------------------------------------------------------
# neighbour search / evaluation
# -------------------------------------------------------------------------------------------


def topk_inner(q, c, dim, k, id_map=None, ws_bytes=None):
    nq, nc = q.shape[0], c.shape[0]
    full = lib().oea_topk_workspace_bytes(nq, nc)
    # default: strips of <= 2 GB.  Measured at 100,000 x 100,000, k = 2,000: 64 MB strips 169 ms, 192 MB (Infinity-
    # Cache resident) 77 ms, 1.5 GB 51 ms, 12 GB 46 ms -- thousands of rows per launch (a full wave of workgroups
    # for both kernels, few launch tails) matter more than keeping the strip in the 256 MB cache.
    # Long candidate lists (nc >= 32,768, nq >= 4,096) take the strip-free path (csrc/topk.hip): ~55 KB of workspace per
    # query row (sample strip + survivor lists); 8 GB covers 100,000 queries in one pass.
    big = nc >= int(os.environ.get("OEA_TOPK_LISTS_MIN", "32768")) and nq >= 4096
    ws_bytes = min(full, max((8 << 30) if big else (2 << 30), 128 * ((nc + 31) // 32 * 32) * 4)) if ws_bytes is None else min(full, ws_bytes)
    if q.data_ptr() == c.data_ptr() and nq == nc:
        # one KG's entities against themselves: the symmetric search (upper-triangle tiles only) wants its lists for ALL rows
        # at once (~0.3 MB per row at k / n = 2 %); taken when it fits in a third of the free memory
        need = int(lib().oea_topk_sym_workspace_bytes(nq, k))
        if need and need <= torch.cuda.mem_get_info(q.device)[0] // 3:
            ws_bytes = max(ws_bytes, need)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=q.device)
    out = torch.empty((nq, k), dtype=torch.int32, device=q.device)
    check(lib().oea_topk_inner(_p(q), nq, q.shape[1], _p(c), nc, c.shape[1], dim, k, _p(id_map), _p(out),
                               _p(ws), ws_bytes, _stream()))
    return out


def topk_rows(s, k, id_map=None, nc=None):
    """k largest of the first nc (default: all) columns of every row of a device similarity strip
    [n, ld] -> int32 [n, k]."""
    out = torch.empty((s.shape[0], k), dtype=torch.int32, device=s.device)
    check(lib().oea_topk_rows(_p(s), s.shape[0], s.shape[1] if nc is None else nc, s.stride(0), k, _p(id_map), _p(out),
                              _stream()))
    return out


def row_rank_select(vals, k, largest, ids=None, want_sel=True, want_kth=False):
    """the k best of every row of a short [n, c <= 1,024] fp32 / fp64 matrix by ranking (ties: earlier column) -> (selected columns
    int32 [n, k] in ascending column order, mapped through ids [n, c] when given; k-th best value [n]) (oea_row_rank_select_*)"""
    assert vals.dim() == 2 and vals.is_contiguous() and vals.dtype in (torch.float32, torch.float64)
    n, c = vals.shape
    sel = torch.empty((n, k), dtype=torch.int32, device=vals.device) if want_sel else None
    kth = torch.empty(n, dtype=vals.dtype, device=vals.device) if want_kth else None
    fn = lib().oea_row_rank_select_f32 if vals.dtype == torch.float32 else lib().oea_row_rank_select_f64
    if ids is not None:
        assert ids.dtype == torch.int32 and ids.is_contiguous() and ids.shape == vals.shape
    check(fn(_p(vals), n, c, vals.stride(0), int(k), int(bool(largest)), _p(ids), 0 if ids is None else ids.stride(0), _p(sel), _p(kth),
             _stream()))
    return sel, kth


def eval_bf16_enabled(n1, n2):
    """the certified bf16 prefilter (oea_rank_eval_bf16) takes the inner-product evaluation (with or without CSLS means) from
    3e8 pairs (~17,000^2) on: its six launches and the exact fix-up cost ~0.1 ms, which the 10,500 test pairs of the 15K
    datasets do not win back inside greedy_alignment (bench r04k: 34.7 vs 38.5 M pairs/s), the 70,000 of the 100K datasets do
    (11.6 vs 7.5 M pairs/s).  OEA_EVAL_BF16=0 keeps the fp32 sweep, OEA_EVAL_BF16_MIN_PAIRS moves the limit."""
    lim = float(os.environ.get('OEA_EVAL_BF16_MIN_PAIRS', '3e8'))
    return os.environ.get('OEA_EVAL_BF16', '1')[:1] != '0' and n1 * n2 >= lim


def rank_eval(e1, e2, dim, metric='inner', csls_r=None, csls_c=None, gold_offset=0, allow_bf16=True):
    """gold of query row i is candidate row gold_offset + i (row-sharded evaluation passes its lo).  allow_bf16=False: the fp32
    sweep whatever the size (rank_eval_bf16's fallback on a record overflow -- an explicit argument instead of a process-global
    re-entrancy flag)."""
    n1, n2 = e1.shape[0], e2.shape[0]
    assert n1 + gold_offset <= n2, "gold of row i is column gold_offset + i <= n2"
    if metric == 'inner' and n1 > 0 and allow_bf16 and eval_bf16_enabled(n1, n2):
        return rank_eval_bf16(e1, e2, dim, gold_offset, csls_r=csls_r, csls_c=csls_c)
    if metric == 'manhattan' and n1 > 0 and n2 >= 2048 and os.environ.get('OEA_L1_EVAL', 'grid') != 'f64':
        return rank_eval_l1_grid(e1, e2, dim, gold_offset, csls_r=csls_r, csls_c=csls_c)
    ws = torch.empty(lib().oea_rank_workspace_bytes(n1), dtype=torch.uint8, device=e1.device)
    rank = torch.empty(n1, dtype=torch.int32, device=e1.device)
    argmax = torch.empty(n1, dtype=torch.int32, device=e1.device)
    check(lib().oea_rank_eval(_p(e1), n1, e1.shape[1], _p(e2), n2, e2.shape[1], dim, METRIC[metric],
                              _p(csls_r), _p(csls_c), int(gold_offset), _p(rank), _p(argmax), _p(ws), _stream()))
    return rank, argmax


class L1Grid:
    """both tables of a manhattan evaluation on ONE 16-bit grid over their common range (oea_quantize_rows_u16), the error
    bound of a grid distance, and -- when they fit a third of the free memory -- the strips of grid distances of the query
    blocks, kept so that the CSLS evaluation (row means, then ranks) computes them once."""

    def __init__(self, e1, e2, dim, block_bytes=2 << 30):
        self.e1, self.e2, self.dim = e1, e2, dim
        lo1, hi1 = torch.aminmax(e1[:, :dim])
        lo2, hi2 = torch.aminmax(e2[:, :dim])
        lo, hi = min(float(lo1), float(lo2)), max(float(hi1), float(hi2))
        self.step = max(hi - lo, 1e-30) / 65535.0
        self.q1 = quantize_rows_u16(e1, dim, lo, 1.0 / self.step)
        self.q2 = self.q1 if e2 is e1 else quantize_rows_u16(e2, dim, lo, 1.0 / self.step)
        # per entry 0.5 step (rintf) + 2 * 65535 * 2^-24 (fp32 roundings of inv_step and of x - lo) + 2^-9 (of the product, < 65536)
        # = 0.5098 steps, two entries per column: 1.0196 dim steps (pressed to 0.98 dim by tests/test_l1_grid_gpu.py)
        self.err = (dim * 1.02 + 1.0) * self.step
        self.ld = (e2.shape[0] + 31) // 32 * 32
        self.rows_per = int(max(128, min(e1.shape[0], block_bytes // (4 * self.ld))))
        self.strips = {}                               # r0 -> strip of query rows [r0, r0 + rows) against all of e2

    def blocks(self):
        n1 = self.e1.shape[0]
        return [(r0, min(self.rows_per, n1 - r0)) for r0 in range(0, n1, self.rows_per)]

    def strip(self, r0, rows, keep=False):
        s = self.strips.get(r0)
        if s is None:
            s = l1_u16_strip(self.q1[r0: r0 + rows], self.q2)
            if keep:
                self.strips[r0] = s
        return s

    def can_keep(self):
        need = 4 * self.ld * self.e1.shape[0]
        return need <= torch.cuda.mem_get_info(self.e1.device)[0] // 3


def pair_l1_sim(q, table, dim, cand):
    """exact manhattan similarities float(1 - d) of the candidate lists cand int32 [nq, c] (sequential fp64 chain) -> fp32 [nq, c]"""
    nq, c = cand.shape
    out = torch.empty((nq, c), dtype=torch.float32, device=q.device)
    check(lib().oea_pair_l1_sim(_p(q), nq, q.shape[1], _p(table), table.shape[0], table.shape[1], dim, _p(cand), c, _p(out), _stream()))
    return out


def l1_grid_topk_means(q_tab, c_tab, qq, qc, dim, k, step, err, margin=32, block_bytes=2 << 30, keep=None, stats=None):
    """mean of the k largest manhattan similarities of every row of q_tab against c_tab (calculate_nearest_k,
    similarity.py:80-83) WITHOUT the fp64 distance of every pair: the k + margin nearest on the 16-bit grid, their exact
    similarities (sequential fp64 chain, rounded to fp32 like sim()), the mean by oea_row_topk_mean on that short list --
    the same values summed in the same order as over the whole row.  Every list is CERTIFIED: no entity outside it can be
    nearer than its farthest member's lower bound, which must not beat the k-th exact value; rows that fail take the
    all-pairs fp64 strip.  keep: an L1Grid whose strips this pass should leave behind (q_tab = its e1)."""
    n, nc = q_tab.shape[0], c_tab.shape[0]
    ld = (nc + 31) // 32 * 32
    rows_per = keep.rows_per if keep is not None else int(max(128, min(n, block_bytes // (4 * ld))))
    out = torch.empty(n, dtype=torch.float32, device=q_tab.device)
    c = min(k + margin, nc)
    bad = torch.zeros(n, dtype=torch.bool, device=q_tab.device)
    for r0 in range(0, n, rows_per):
        rows = min(rows_per, n - r0)
        strip = keep.strip(r0, rows, keep=True) if keep is not None else l1_u16_strip(qq[r0: r0 + rows], qc)
        cand = topk_rows(strip, c, nc=nc)                                            # the c smallest grid distances
        worst = -torch.gather(strip, 1, cand.to(torch.int64)).amin(dim=1).to(torch.float64)
        qb = q_tab[r0: r0 + rows]
        sims = pair_l1_sim(qb, c_tab, dim, cand)
        out[r0: r0 + rows] = row_topk_mean(sims, k)
        _, kth = row_rank_select(sims, k, True, want_sel=False, want_kth=True)       # the k-th largest exact similarity of the list
        # a non-member's distance is at least worst * step - err (+ 4 steps: float rounding of large grid sums)
        bound = 1.0 - (worst * step - (err + 4.0 * step))
        if c < nc:
            bad[r0: r0 + rows] = ~(bound <= kth.to(torch.float64))
        del strip
    redo = torch.nonzero(bad).reshape(-1)                    # ONE host read per call (was one per block of rows)
    redone = int(redo.numel())
    for b0 in range(0, redone, 4096):                        # uncertified rows: the all-pairs fp64 strip
        idx = redo[b0: b0 + 4096]
        s = sim_matrix(q_tab.index_select(0, idx).contiguous(), c_tab, dim, 'manhattan')
        out[idx] = row_topk_mean(s, k)
        del s
    if stats is not None:
        stats['uncertified'] = stats.get('uncertified', 0) + redone
    return out


def csls_means_l1_grid(e1, e2, dim, k, cols=True):
    """CSLS means of the manhattan metric from grid distances -> (r [n1], c [n2] or None, grid): the L1Grid keeps the query
    strips (when they fit) for rank_eval_l1_grid(..., grid=grid)."""
    grid = L1Grid(e1, e2, dim)
    keep = grid if (cols and grid.can_keep()) else None        # the strips are kept for the single-process rank pass only
    r = l1_grid_topk_means(e1, e2, grid.q1, grid.q2, dim, k, grid.step, grid.err, keep=keep)
    c = l1_grid_topk_means(e2, e1, grid.q2, grid.q1, dim, k, grid.step, grid.err) if cols else None
    return r, c, grid


def sim_bf16_matrix(e1, e2, dim):
    """the bf16 prefilter's approximate inner products (tests / timing) -> fp32 [n1, n2]"""
    n1, n2 = e1.shape[0], e2.shape[0]
    out = torch.empty((n1, n2), dtype=torch.float32, device=e1.device)
    check(lib().oea_sim_bf16_matrix(_p(e1), n1, e1.shape[1], _p(e2), n2, e2.shape[1], dim, _p(out), n2, _stream()))
    return out


def rank_eval_bf16(e1, e2, dim, gold_offset=0, stats=None, csls_r=None, csls_c=None):
    """rank_eval(metric='inner') through the certified bf16 prefilter (oea_rank_eval_bf16[_csls]): the same rank / argmax, the
    matrix work at 3/16 of the fp32 matrix time.  Falls back to the fp32 sweep when the record buffer overflows (one host read
    of the status word).  stats: optional dict, receives 'records' and 'fallback'."""
    n1 = e1.shape[0]
    ws = torch.empty(lib().oea_rank_eval_bf16_workspace_bytes(n1, dim), dtype=torch.uint8, device=e1.device)
    rank = torch.empty(n1, dtype=torch.int32, device=e1.device)
    argmax = torch.empty(n1, dtype=torch.int32, device=e1.device)
    status = torch.zeros(2, dtype=torch.int32, device=e1.device)
    check(lib().oea_rank_eval_bf16_csls(_p(e1), n1, e1.shape[1], _p(e2), e2.shape[0], e2.shape[1], dim, _p(csls_r), _p(csls_c),
                                        int(gold_offset), _p(rank), _p(argmax), _p(status), _p(ws), _stream()))
    st = status.cpu().numpy()
    if stats is not None:
        stats['records'], stats['fallback'] = int(st[1]), bool(st[0])
    if st[0]:
        return rank_eval(e1, e2, dim, 'inner', csls_r, csls_c, gold_offset=gold_offset, allow_bf16=False)
    return rank, argmax


def rank_eval_metrics_bf16(e1, e2, dim, top_k, gold_offset=0, stats=None, csls_r=None, csls_c=None):
    """rank_eval_metrics through the certified bf16 prefilter: six launches + ONE device->host copy that carries the metrics and
    the sweep's status -> (rank, argmax, hits, rank_sum, rr_sum), or None when the record buffer overflowed (the caller takes
    the fp32 sweep)."""
    n1, nk = e1.shape[0], len(top_k)
    ws = torch.empty(lib().oea_rank_eval_bf16_workspace_bytes(n1, dim), dtype=torch.uint8, device=e1.device)
    rank = torch.empty(n1, dtype=torch.int32, device=e1.device)
    argmax = torch.empty(n1, dtype=torch.int32, device=e1.device)
    buf = torch.empty(nk + 4, dtype=torch.int64, device=e1.device)
    tk = (C.c_int32 * nk)(*[int(k) for k in top_k])
    check(lib().oea_rank_eval_metrics_bf16(_p(e1), n1, e1.shape[1], _p(e2), e2.shape[0], e2.shape[1], dim, _p(csls_r), _p(csls_c),
                                           int(gold_offset), tk, nk, _p(rank), _p(argmax), C.c_void_p(buf.data_ptr()), _p(ws), _stream()))
    host = buf.cpu().numpy()
    if stats is not None:
        stats['records'], stats['fallback'] = int(host[nk + 3]), bool(host[nk + 2])
    if host[nk + 2]:
        return None
    return rank, argmax, [int(x) for x in host[:nk]], int(host[nk]), float(host[nk + 1:nk + 2].view(np.float64)[0])


def rank_eval_l1_grid(e1, e2, dim, gold_offset=0, block_bytes=2 << 30, csls_r=None, csls_c=None, grid=None):
    """rank_eval(metric='manhattan') without the fp64 distance of every pair: 16-bit grid distances of all pairs
    (oea_l1_u16_strip, blocks of query rows), then oea_rank_l1_grid_rows[_csls] -- exact similarities only where the grid
    leaves a doubt.  Same ranks and nearest candidates as the all-pairs fp64 kernel (tested), with or without CSLS means."""
    n1, n2 = e1.shape[0], e2.shape[0]
    if grid is None or grid.e1.data_ptr() != e1.data_ptr() or grid.e2.data_ptr() != e2.data_ptr() or grid.e1.shape != e1.shape:
        grid = L1Grid(e1, e2, dim, block_bytes)
    step, err, ld = grid.step, grid.err, grid.ld
    rank = torch.empty(n1, dtype=torch.int32, device=e1.device)
    argmax = torch.empty(n1, dtype=torch.int32, device=e1.device)
    n_exact = torch.zeros(1, dtype=torch.int32, device=e1.device)
    csls = csls_r is not None
    for r0, rows in grid.blocks():
        strip = grid.strip(r0, rows)
        if csls:
            check(lib().oea_rank_l1_grid_rows_csls(_p(strip), rows, r0, n2, ld, _p(e1), e1.shape[1], _p(e2), e2.shape[1], dim,
                                                   int(gold_offset), float(step), float(err), _p(csls_r), _p(csls_c), _p(rank),
                                                   _p(argmax), _p(n_exact), _stream()))
        else:
            check(lib().oea_rank_l1_grid_rows(_p(strip), rows, r0, n2, ld, _p(e1), e1.shape[1], _p(e2), e2.shape[1], dim,
                                              int(gold_offset), float(step), float(err), _p(rank), _p(argmax), _p(n_exact), _stream()))
        del strip
        grid.strips.pop(r0, None)
        r1 = r0 + rows
        if r0 == 0 and r1 < n1 and int(n_exact.item()) > rows // 64:
            # the grid is useless for this table (outliers stretch its range: most candidates are within the error bound of
            # the gold distance and whole rows fall back to exact pairs): the rest through the all-pairs fp64 kernel
            rest = n1 - r1
            ws = torch.empty(lib().oea_rank_workspace_bytes(rest), dtype=torch.uint8, device=e1.device)
            rk, am = torch.empty(rest, dtype=torch.int32, device=e1.device), torch.empty(rest, dtype=torch.int32, device=e1.device)
            check(lib().oea_rank_eval(_p(e1[r1:]), rest, e1.shape[1], _p(e2), n2, e2.shape[1], dim, METRIC['manhattan'],
                                      _p(csls_r[r1:].contiguous()) if csls else None, _p(csls_c), int(gold_offset) + r1, _p(rk), _p(am),
                                      _p(ws), _stream()))
            rank[r1:], argmax[r1:] = rk, am
            grid.strips.clear()
            break
    return rank, argmax


def rank_eval_metrics(e1, e2, dim, top_k, csls_r=None, csls_c=None, gold_offset=0):
    """inner-product evaluation in two launches (oea_rank_eval_metrics) + ONE device->host copy ->
    (rank int32 [n1] device, argmax int32 [n1] device, hits counts list[int], rank_sum int, rr_sum float)."""
    n1, n2 = e1.shape[0], e2.shape[0]
    assert n1 + gold_offset <= n2, "gold of row i is column gold_offset + i <= n2"
    nk = len(top_k)
    ws = torch.empty(lib().oea_rank_eval_metrics_workspace_bytes(n1), dtype=torch.uint8, device=e1.device)
    rank = torch.empty(n1, dtype=torch.int32, device=e1.device)
    argmax = torch.empty(n1, dtype=torch.int32, device=e1.device)
    buf = torch.empty(nk + 2, dtype=torch.int64, device=e1.device)     # hits[nk], rank_sum, rr bits: all written by the kernel
    tk = (C.c_int32 * nk)(*[int(k) for k in top_k])
    check(lib().oea_rank_eval_metrics(_p(e1), n1, e1.shape[1], _p(e2), n2, e2.shape[1], dim, _p(csls_r), _p(csls_c),
                                      int(gold_offset), tk, nk, _p(rank), _p(argmax), C.c_void_p(buf.data_ptr()),
                                      C.c_void_p(buf.data_ptr() + 8 * (nk + 1)), _p(ws), _stream()))
    host = buf.cpu().numpy()
    return rank, argmax, [int(x) for x in host[:nk]], int(host[nk]), float(host[nk + 1:nk + 2].view(np.float64)[0])


def rank_rows(s, gold_idx):
    """rank of column gold_idx[i] in row i of a device similarity block + row argmax -> (int32[n], int32[n])."""
    n = s.shape[0]
    rank = torch.empty(n, dtype=torch.int32, device=s.device)
    argmax = torch.empty(n, dtype=torch.int32, device=s.device)
    check(lib().oea_rank_rows(_p(s), n, s.shape[1], s.stride(0), _p(gold_idx), _p(rank), _p(argmax), _stream()))
    return rank, argmax


def rank_metrics(rank, top_k):
    """-> (hits counts list[int], rank_sum int, rr_sum float) with ONE device->host copy."""
    nk = len(top_k)
    tk = (C.c_int32 * nk)(*[int(k) for k in top_k])
    buf = torch.zeros(nk + 2, dtype=torch.int64, device=rank.device)   # hits[nk], rank_sum, rr bits
    check(lib().oea_rank_metrics(_p(rank), rank.numel(), tk, nk, C.c_void_p(buf.data_ptr()),
                                 C.c_void_p(buf.data_ptr() + 8 * nk), C.c_void_p(buf.data_ptr() + 8 * (nk + 1)),
                                 _stream()))
    host = buf.cpu().numpy()
    hits = [int(x) for x in host[:nk]]
    return hits, int(host[nk]), float(host[nk + 1:nk + 2].view(np.float64)[0])


def sim_matrix(e1, e2, dim, metric='inner', pad=False):
    """-> device fp32 [n1, n2]; pad=True: [n1, ld] with ld = n2 rounded up to 32 (the row layout that
    topk_rows reads; columns n2.. are left unwritten)."""
    n1, n2 = e1.shape[0], e2.shape[0]
    ld = (n2 + 31) // 32 * 32 if pad else n2
    out = torch.empty((n1, ld), dtype=torch.float32, device=e1.device)
    check(lib().oea_sim_matrix(_p(e1), n1, e1.shape[1], _p(e2), n2, e2.shape[1], dim, METRIC[metric],
                               _p(out), ld, _stream()))
    return out


def quantize_rows_u16(table, dim, lo, inv_step):
    """-> int16-typed device tensor [n, ldq] holding u16 grid points (ldq = dim rounded up to 8; pad columns 0)."""
    n = table.shape[0]
    ldq = (dim + 7) // 8 * 8
    out = torch.empty((n, ldq), dtype=torch.int16, device=table.device)
    check(lib().oea_quantize_rows_u16(_p(table), n, table.shape[1], dim, float(lo), float(inv_step), _p(out), ldq, _stream()))
    return out


def l1_u16_strip(qq, qc, pad=True):
    """-> device fp32 [nq, ld]: minus the integer L1 distance of every (query, candidate) pair of two u16 row sets."""
    nq, nc = qq.shape[0], qc.shape[0]
    ld = (nc + 31) // 32 * 32 if pad else nc
    out = torch.empty((nq, ld), dtype=torch.float32, device=qq.device)
    check(lib().oea_l1_u16_strip(_p(qq), nq, _p(qc), nc, qq.shape[1], _p(out), ld, _stream()))
    return out


def pair_l1_f64(q, table, dim, cand):
    """exact fp64 L1 distances of the candidate lists cand int32 [nq, c] -> fp64 [nq, c]."""
    nq, c = cand.shape
    out = torch.empty((nq, c), dtype=torch.float64, device=q.device)
    check(lib().oea_pair_l1_f64(_p(q), nq, q.shape[1], _p(table), table.shape[0], table.shape[1], dim, _p(cand), c, _p(out),
                                _stream()))
    return out


def row_topk_mean(s, k):
    out = torch.empty(s.shape[0], dtype=torch.float32, device=s.device)
    check(lib().oea_row_topk_mean(_p(s), s.shape[0], s.shape[1], s.stride(0), k, _p(out), _stream()))
    return out


def csls_means(e1, e2, dim, k):
    """one-sweep CSLS means (oea_csls_means) -> (r [n1], c [n2]) or None when the shape is not covered"""
    n1, n2 = e1.shape[0], e2.shape[0]
    nbytes = lib().oea_csls_means_workspace_bytes(n1, n2, int(k))
    if nbytes == 0:
        return None
    ws = torch.empty(nbytes, dtype=torch.uint8, device=e1.device)
    r = torch.empty(n1, dtype=torch.float32, device=e1.device)
    c = torch.empty(n2, dtype=torch.float32, device=e1.device)
    check(lib().oea_csls_means(_p(e1), n1, e1.shape[1], _p(e2), n2, e2.shape[1], dim, int(k), _p(r), _p(c), _p(ws), nbytes, _stream()))
    return r, c


def csls_apply_(s, r, c):
    check(lib().oea_csls_apply(_p(s), s.shape[0], s.shape[1], s.stride(0), _p(r), _p(c), _stream()))
    return s


# -------------------------------------------------------------------------------------------
# graph builders (csrc/graph_build.hip): triples in, sorted COO out (host numpy: the operands are cut into CSR / chunk
# layouts by the constructors of models/graph_ops.py afterwards)
# -------------------------------------------------------------------------------------------


def _triples_dev(triples, dev=None):
    """list / set iteration order / ndarray [n, 3] -> device int32 [n, 3]"""
    if isinstance(triples, torch.Tensor):
        return triples.to(dtype=torch.int32).contiguous()
    if isinstance(triples, np.ndarray):
        a = np.ascontiguousarray(triples, dtype=np.int32).reshape(-1, 3)
    else:
        a = np.fromiter((x for tr in triples for x in tr), np.int32, count=3 * len(triples)).reshape(-1, 3)
    return torch.from_numpy(a).to(dev or device())


def _coo_out(cap, dev, val_dtype):
    return (torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev),
            torch.empty(cap, dtype=val_dtype, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))


def build_unweighted_adj(triples, n_ent):
    """alinet.py:155-181 -> (row, col, val fp64) numpy, sorted by (row, col)."""
    tri = _triples_dev(triples)
    n = tri.shape[0]
    cap = 2 * n + int(n_ent)
    row, col, val, nnz = _coo_out(cap, tri.device, torch.float64)
    check(lib().oea_build_unweighted_adj(_p(tri), n, int(n_ent), _p(row), _p(col), _p(val), cap, _p(nnz), _stream()))
    m = int(nnz.item())
    return row[:m].cpu().numpy(), col[:m].cpu().numpy(), val[:m].cpu().numpy()


def build_weighted_adj(triples, n_ent, n_rel, raw=False):
    """gcn_align.py:610-664 + 566-578 -> dict(r2f, r2if [n_rel], support = (row, col, val), adj = (row, col, val) if raw)."""
    tri = _triples_dev(triples)
    n = tri.shape[0]
    dev = tri.device
    cap = 2 * n + int(n_ent)
    r2f = torch.zeros(int(n_rel), dtype=torch.float64, device=dev)
    r2if = torch.zeros(int(n_rel), dtype=torch.float64, device=dev)
    row, col, val, nnz = _coo_out(cap, dev, torch.float64)
    a_row, a_col, a_val, a_nnz = _coo_out(cap, dev, torch.float64) if raw else (None, None, None, None)
    check(lib().oea_build_weighted_adj(_p(tri), n, int(n_ent), int(n_rel), _p(r2f), _p(r2if), _p(a_row), _p(a_col), _p(a_val),
                                       _p(a_nnz), _p(row), _p(col), _p(val), cap, _p(nnz), _stream()))
    m = int(nnz.item())
    out = dict(r2f=r2f.cpu().numpy(), r2if=r2if.cpu().numpy(),
               support=(row[:m].cpu().numpy(), col[:m].cpu().numpy(), val[:m].cpu().numpy()))
    if raw:
        ma = int(a_nnz.item())
        out["adj"] = (a_row[:ma].cpu().numpy(), a_col[:ma].cpu().numpy(), a_val[:ma].cpu().numpy())
    return out


def build_primal_adj(triples, n_ent):
    """rdgcn.py:45-72 -> (row, col, val fp32) numpy."""
    tri = _triples_dev(triples)
    n = tri.shape[0]
    cap = 2 * n + int(n_ent)
    row, col, val, nnz = _coo_out(cap, tri.device, torch.float32)
    check(lib().oea_build_primal_adj(_p(tri), n, int(n_ent), _p(row), _p(col), _p(val), cap, _p(nnz), _stream()))
    m = int(nnz.item())
    return row[:m].cpu().numpy(), col[:m].cpu().numpy(), val[:m].cpu().numpy()


def build_dual_adj(triples, n_rel):
    """rdgcn.py:17-42 + 268-277 -> device fp32 [n_rel, n_rel]."""
    tri = _triples_dev(triples)
    out = torch.empty((int(n_rel), int(n_rel)), dtype=torch.float32, device=tri.device)
    check(lib().oea_build_dual_adj(_p(tri), tri.shape[0], int(n_rel), _p(out), _stream()))
    return out


def build_2hop(triples, full_triples, n_ent, n_rel, n_cut=5):
    """alinet.py:250-287 -> (int64 [m, 3] numpy sorted by (h, r, t), stats = the reference's four log counts)."""
    tri = _triples_dev(triples)
    full = tri if full_triples is None else _triples_dev(full_triples)
    n = tri.shape[0]
    stats = (C.c_int64 * 4)()
    n_out = torch.zeros(1, dtype=torch.int64, device=tri.device)
    cap = max(4 * n, 1 << 16)
    while True:
        out = torch.empty((cap, 3), dtype=torch.int32, device=tri.device)
        rc = lib().oea_build_2hop(_p(tri), n, _p(full), full.shape[0], int(n_ent), int(n_rel), int(n_cut), _p(out), cap, _p(n_out),
                                  stats, _stream())
        m = int(n_out.item())
        if rc != 0 and m > cap:            # the count is known now: once more with room for it
            cap = m
            continue
        check(rc)
        return out[:m].cpu().numpy().astype(np.int64), [int(x) for x in stats]


# -------------------------------------------------------------------------------------------
# graph aggregate
# -------------------------------------------------------------------------------------------


def csr_split(indptr, threshold=768, chunk=512, dev=None, row_range=None):
    """host CSR row pointer -> oea_csr_split for rows with more than `threshold` nonzeros (None if there
    are none): each such row is cut into chunks of `chunk` nonzeros.  row_range=(lo, hi): only rows of
    that block, numbered relative to lo (a rank's block of a row-sharded aggregate)."""
    indptr = np.asarray(indptr, np.int64)
    lens = np.diff(indptr)
    lo, hi = row_range if row_range is not None else (0, len(lens))
    rows = np.flatnonzero(lens[lo:hi] > threshold)
    if len(rows) == 0:
        return None
    c_row, c_e0, c_e1, first = [], [], [], []
    for r in rows:
        first.append(len(c_row))
        for e0 in range(int(indptr[lo + r]), int(indptr[lo + r + 1]), chunk):
            c_row.append(r)
            c_e0.append(e0)
            c_e1.append(min(e0 + chunk, int(indptr[lo + r + 1])))
    first.append(len(c_row))
    t = [to_ids(np.asarray(a, np.int32), dev) for a in (c_row, c_e0, c_e1, rows, first)]
    tickets = torch.zeros(len(rows), dtype=torch.int32, device=t[0].device)      # last-arriver tickets of the hub rows (self-resetting)
    sp_ = _lib.CsrSplit(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), len(c_row), len(rows), int(threshold),
                        t[4].data_ptr(), None, 0, tickets.data_ptr())
    sp_._keep = t + [tickets]
    return sp_


def _split_partials(split, ld, dev):
    """grow-only buffer for the hub chunks' partial sums (stream-ordered reuse by the calls on this operand)"""
    need = int(split.n_chunks) * int(ld)
    if split.partials_floats < need:
        buf = torch.empty(need, dtype=torch.float32, device=dev)
        split._partials = buf
        split.partials, split.partials_floats = buf.data_ptr(), need
    return split


def spmm_csr(rowptr, colidx, vals, x, dim, act=0, mask_from=None, out=None, split=None):
    n_rows = rowptr.numel() - 1
    if out is None:
        out = torch.empty((n_rows, x.shape[1]), dtype=torch.float32, device=x.device)
    if split is not None:
        _split_partials(split, out.shape[1], x.device)
    check(lib().oea_spmm_csr(_p(rowptr), _p(colidx), _p(vals), n_rows, _p(x), dim, x.shape[1], int(act),
                             _p(mask_from), _p(out), out.shape[1], C.byref(split) if split is not None else None,
                             _stream()))
    return out


def align_loss_l1(out_emb, dim, ill, k, gamma, neg_left, neg_right, neg2_left, neg2_right, grad, loss_accum):
    check(lib().oea_align_loss_l1(_p(out_emb), out_emb.shape[0], dim, out_emb.shape[1], _p(ill), ill.shape[0],
                                  k, float(gamma), _p(neg_left), _p(neg_right), _p(neg2_left), _p(neg2_right),
                                  _p(grad), _p(loss_accum), _stream()))


def sgd_rows_(w, grad_t, dim, normalize, lr):
    check(lib().oea_sgd_rows(_p(w), _p(grad_t), w.shape[0], dim, w.shape[1], int(bool(normalize)), float(lr), _stream()))
    return w


# -------------------------------------------------------------------------------------------
# sparse graph attention + dense Adam
# -------------------------------------------------------------------------------------------


ATTN_ALPHA, ATTN_AGGREGATE, ATTN_DZ, ATTN_DV = 1, 2, 1, 2


def attn_graph(sub_ptr, sub_seg, seg_sub_ptr, seg_row, colidx, agg_rowptr, agg_colidx, agg_edge, t_rowptr, t_row, t_edge,
               agg_split=None, t_split=None, seg_range=None, sub_range=None, agg_rows=None, agg_slots=None, t_rows=None,
               t_slots=None):
    """pack the device arrays of an attention graph (keeps them alive).  agg_edge None: the edge order is the
    aggregate's CSR order.  The *_range / *_rows / *_slots arguments restrict the ranges a call works on (a rank's blocks
    of a row-sharded job); default: the whole graph."""
    n_sub, n_seg = sub_seg.numel(), seg_row.numel()
    n_agg, n_t, nnz = agg_rowptr.numel() - 1, t_rowptr.numel() - 1, colidx.numel()
    s0, s1 = sub_range if sub_range is not None else (0, n_sub)
    g0, g1 = seg_range if seg_range is not None else (0, n_seg)
    a0, a1 = agg_rows if agg_rows is not None else (0, n_agg)
    as0, as1 = agg_slots if agg_slots is not None else (0, nnz)
    t0, t1 = t_rows if t_rows is not None else (0, n_t)
    ts0, ts1 = t_slots if t_slots is not None else (0, nnz)
    g = _lib.AttnGraph(sub_ptr.data_ptr(), sub_seg.data_ptr(), seg_sub_ptr.data_ptr(), seg_row.data_ptr(), colidx.data_ptr(),
                       n_sub, n_seg, nnz, agg_rowptr.data_ptr(), agg_colidx.data_ptr(),
                       agg_edge.data_ptr() if agg_edge is not None else None, n_agg,
                       C.pointer(agg_split) if agg_split is not None else None,
                       t_rowptr.data_ptr(), t_row.data_ptr(), t_edge.data_ptr(), n_t,
                       C.pointer(t_split) if t_split is not None else None,
                       int(s0), int(s1), int(g0), int(g1), int(a0), int(a1), int(as0), int(as1), int(t0), int(t1), int(ts0), int(ts1))
    g._keep = (sub_ptr, sub_seg, seg_sub_ptr, seg_row, colidx, agg_rowptr, agg_colidx, agg_edge, t_rowptr, t_row, t_edge,
               agg_split, t_split)
    g._splits = (agg_split, t_split)
    return g


def _attn_ws(g, ld, dev):
    for sp_ in g._splits:
        if sp_ is not None:
            _split_partials(sp_, ld, dev)
    return torch.empty(lib().oea_sparse_attn_workspace_floats(C.byref(g)), dtype=torch.float32, device=dev)


def sparse_attn_fwd(g, z, v, dim, slope, n_rows, out=None, alpha=None, phases=ATTN_ALPHA | ATTN_AGGREGATE):
    """-> (out [n_rows, ld], alpha [nnz]); every row / edge of the graph's ranges is written (no zero-fill needed for a
    whole-graph call; a sharded caller passes its own out / alpha)."""
    if out is None:
        out = torch.empty((n_rows, v.shape[1]), dtype=torch.float32, device=v.device)
    if alpha is None:
        alpha = torch.empty_like(z)
    ws = _attn_ws(g, v.shape[1], v.device)
    check(lib().oea_sparse_attn_fwd(C.byref(g), _p(z), _p(v), dim, v.shape[1], float(slope), _p(out), _p(alpha), _p(ws),
                                    int(phases), _stream()))
    return out, alpha


def sparse_attn_bwd(g, z, v, alpha, dout, dim, slope, dz=None, dv=None, phases=ATTN_DZ | ATTN_DV):
    """-> (dz [nnz], dv [n_cols, ld])."""
    if dz is None:
        dz = torch.empty_like(z)
    if dv is None:
        dv = torch.empty_like(v)
    ws = _attn_ws(g, v.shape[1], v.device)
    check(lib().oea_sparse_attn_bwd(C.byref(g), _p(z), _p(v), _p(alpha), _p(dout), dim, v.shape[1], float(slope), _p(dz),
                                    _p(dv), _p(ws), int(phases), _stream()))
    return dz, dv


def sparse_attn_dz_(g, z, alpha, dalpha, slope, ld):
    """d alpha per edge (overwritten) -> d z per edge, over the graph's softmax groups (oea_sparse_attn_dz)"""
    ws = _attn_ws(g, ld, z.device)
    check(lib().oea_sparse_attn_dz(C.byref(g), _p(z), _p(alpha), _p(dalpha), float(slope), _p(ws), _stream()))
    return dalpha


def adam_dense_(param, grad, m, v, lr, t, beta1=0.9, beta2=0.999, eps=1e-8):
    check(lib().oea_adam_dense(_p(param), _p(grad), _p(m), _p(v), param.numel(), float(lr), float(beta1), float(beta2),
                               float(eps), int(t), _stream()))
    return param


# -------------------------------------------------------------------------------------------
# fused row-wise glue of the GNN approaches (csrc/gnn_fused.hip)
# -------------------------------------------------------------------------------------------


def _ptr_array(tensors):
    arr = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    return arr


def _i32_array(vals):
    return (C.c_int32 * len(vals))(*[int(v) for v in vals])


def concat_l2n_fwd(xs):
    """xs: list of <= 4 contiguous [n, d_i] fp32 tensors -> (emb [n, pad4(sum d)], inv_blk [n, 4], inv_all [n])."""
    n = xs[0].shape[0]
    dims = [x.shape[1] for x in xs]
    out = torch.empty((n, pad4(sum(dims))), dtype=torch.float32, device=xs[0].device)
    inv_blk = torch.empty((n, 4), dtype=torch.float32, device=out.device)
    inv_all = torch.empty(n, dtype=torch.float32, device=out.device)
    check(lib().oea_concat_l2n_fwd(_ptr_array(xs), _i32_array(dims), _i32_array(dims), len(xs), n, _p(out), out.shape[1],
                                   _p(inv_blk), _p(inv_all), _stream()))
    return out, inv_blk, inv_all


def concat_l2n_bwd(dims, z, dz, inv_blk, inv_all):
    n = z.shape[0]
    dxs = [torch.empty((n, d), dtype=torch.float32, device=z.device) for d in dims]
    check(lib().oea_concat_l2n_bwd(_ptr_array(dxs), _i32_array(dims), _i32_array(dims), len(dims), n, _p(z), _p(dz), z.shape[1],
                                   _p(inv_blk), _p(inv_all), _stream()))
    return dxs


def pair_loss_l2_fwd(emb, dim, pairs, n_pos, weight, margin, balance):
    """pairs int32 [m, 2] (the first n_pos positive) -> (terms [m], coef [m])."""
    m = pairs.shape[0]
    coef = torch.empty(m, dtype=torch.float32, device=emb.device)
    terms = torch.empty(m, dtype=torch.float32, device=emb.device)
    check(lib().oea_pair_loss_l2_fwd(_p(emb), emb.shape[0], dim, emb.shape[1], _p(pairs), m, int(n_pos), _p(weight), float(margin),
                                     float(balance), _p(coef), _p(terms), _stream()))
    return terms, coef


def pair_rows_csr(pairs, n_rows):
    """the endpoints of `pairs` (device int [m, 2]) grouped by row, slots in pair order (oea_pair_rows_build: one stable
    device sort + a scan, no host synchronisation) -> (rowptr int32 [n_rows + 1], other int32 [2 m], slot_pair int32 [2 m])
    for pair_grad_rows."""
    pairs = pairs.to(torch.int32).contiguous()
    m = pairs.shape[0]
    rowptr = torch.empty(n_rows + 1, dtype=torch.int32, device=pairs.device)
    other = torch.empty(2 * m, dtype=torch.int32, device=pairs.device)
    slot_pair = torch.empty(2 * m, dtype=torch.int32, device=pairs.device)
    check(lib().oea_pair_rows_build(_p(pairs), m, int(n_rows), _p(rowptr), _p(other), _p(slot_pair), _stream()))
    return rowptr, other, slot_pair


def pair_grad_rows(emb, dim, rowptr, other, slot_pair, coef, gscale=None, norm=2, out=None):
    """grad[r] = gscale * sum over row r's pair slots of 2 coef (e_r - e_other) (norm 2) | coef sign(e_r - e_other) (norm 1)."""
    grad = torch.empty_like(emb) if out is None else out
    check(lib().oea_pair_grad_rows(_p(emb), emb.shape[0], dim, emb.shape[1], _p(rowptr), _p(other), _p(slot_pair), _p(coef),
                                   _p(gscale), int(norm), _p(grad), _stream()))
    return grad


def align_loss_l1_coef(out_emb, dim, ill, k, gamma, neg_left, neg_right, neg2_left, neg2_right, loss_accum, coef=None):
    """the L1 hinge without its gradient -> coef [t + 2 t k] (signed pair coefficients for pair_grad_rows(norm=1))."""
    t = ill.shape[0]
    if coef is None:
        coef = torch.empty(t + 2 * t * k, dtype=torch.float32, device=out_emb.device)
    check(lib().oea_align_loss_l1_coef(_p(out_emb), out_emb.shape[0], dim, out_emb.shape[1], _p(ill), t, k, float(gamma),
                                       _p(neg_left), _p(neg_right), _p(neg2_left), _p(neg2_right), None, _p(loss_accum), _p(coef),
                                       _stream()))
    return coef


def highway_fwd(a, b, p, gamma, beta):
    out = torch.empty_like(a)
    check(lib().oea_highway_fwd(_p(a), _p(b), _p(p), _p(gamma), _p(beta), a.shape[0], a.shape[1], _p(out), _stream()))
    return out


def highway_bwd(a, b, p, gamma, beta, out, gout):
    n, d = a.shape
    da, db, dp = torch.empty_like(a), torch.empty_like(a), torch.empty_like(a)
    parts = torch.empty((lib().oea_colsum_blocks(n), 2, d), dtype=torch.float32, device=a.device)
    check(lib().oea_highway_bwd(_p(a), _p(b), _p(p), _p(gamma), _p(beta), _p(out), _p(gout), n, d, _p(da), _p(db), _p(dp), _p(parts),
                                _stream()))
    sums = parts.sum(0)
    return da, db, dp, sums[0], sums[1]


def gemm_tn(a, b):
    """a^T @ b for two tall row-major fp32 matrices with the same number of rows -> [a.shape[1], b.shape[1]]
    (oea_gemm_tn_f32; shapes it does not take -- widths not multiples of 4 -- go to the library)."""
    m, k1 = a.shape
    k2 = b.shape[1]
    if k1 % 4 or k2 % 4 or not (a.is_contiguous() and b.is_contiguous()) or a.data_ptr() % 16 or b.data_ptr() % 16:
        return a.t() @ b
    out = torch.empty((k1, k2), dtype=torch.float32, device=a.device)
    n_ws = lib().oea_gemm_tn_workspace_floats(m, k1, k2)
    ws = torch.empty(n_ws, dtype=torch.float32, device=a.device) if n_ws else None
    check(lib().oea_gemm_tn_f32(_p(a), k1, k1, _p(b), k2, k2, m, _p(out), k2, _p(ws), _stream()))
    return out


def gemm_tn_sharded(a, b, rank, world, allgather_blocks):
    """a^T @ b in a job whose ranks share the work by ROW CHUNKS (include/openea_hip.h: oea_gemm_tn_partial / _reduce): this
    rank's chunks, one all-gather of the chunk partials (allgather_blocks(full [chunks, k1*k2], bounds)), then all chunks
    added in chunk order -- bit-identical with gemm_tn on one process.  Falls back to the replicated product when the shape
    does not take the kernel or has fewer chunks than ranks."""
    m, k1 = a.shape
    k2 = b.shape[1]
    if (world <= 1 or m == 0 or k1 % 4 or k2 % 4 or not (a.is_contiguous() and b.is_contiguous()) or a.data_ptr() % 16
            or b.data_ptr() % 16):
        return gemm_tn(a, b)
    chunks, rpc = C.c_int32(0), C.c_int64(0)
    check(lib().oea_gemm_tn_plan(m, k1, k2, C.byref(chunks), C.byref(rpc)))
    chunks = chunks.value
    if chunks < world:
        return gemm_tn(a, b)
    bounds = [chunks * r // world for r in range(world + 1)]
    ws = torch.empty((chunks, k1 * k2), dtype=torch.float32, device=a.device)
    check(lib().oea_gemm_tn_partial(_p(a), k1, k1, _p(b), k2, k2, m, bounds[rank], bounds[rank + 1], _p(ws), _stream()))
    allgather_blocks(ws, bounds)
    out = torch.empty((k1, k2), dtype=torch.float32, device=a.device)
    check(lib().oea_gemm_tn_reduce(_p(ws), chunks, k1, k2, _p(out), k2, _stream()))
    return out


def sigmoid_mix_fwd(a, b, p, bias):
    out = torch.empty_like(a)
    check(lib().oea_sigmoid_mix_fwd(_p(a), _p(b), _p(p), _p(bias), a.shape[0], a.shape[1], _p(out), _stream()))
    return out


def sigmoid_mix_bwd(a, b, p, bias, gout, b_relu=False):
    """-> da, db, dp, dbias (db gated by b > 0 when b is a relu's output)"""
    n, d = a.shape
    da, db, dp = torch.empty_like(a), torch.empty_like(a), torch.empty_like(a)
    parts = torch.empty((lib().oea_colsum_blocks(n), d), dtype=torch.float32, device=a.device)
    check(lib().oea_sigmoid_mix_bwd(_p(a), _p(b), _p(p), _p(bias), _p(gout), n, d, int(bool(b_relu)), _p(da), _p(db), _p(dp),
                                    _p(parts), _stream()))
    return da, db, dp, parts.sum(0)


def relu_axpy_fwd(x, y, alpha):
    out = torch.empty_like(x)
    check(lib().oea_relu_axpy_fwd(_p(x), _p(y), float(alpha), x.numel(), _p(out), _stream()))
    return out


def relu_axpy_bwd(y, gout, alpha):
    dy = torch.empty_like(y)
    check(lib().oea_relu_axpy_bwd(_p(y), _p(gout), float(alpha), y.numel(), _p(dy), _stream()))
    return dy


def colsum_prod(x, y):
    """column sums of x * y -> fp32 [d] (fixed order: row blocks, then blocks)"""
    n, d = x.shape
    parts = torch.empty((lib().oea_colsum_blocks(n), d), dtype=torch.float32, device=x.device)
    check(lib().oea_colsum_prod(_p(x), _p(y), n, d, _p(parts), _stream()))
    return parts.sum(0)


def bias_tanh_fwd(x, bias):
    y = torch.empty_like(x)
    check(lib().oea_bias_tanh_fwd(_p(x), _p(bias), x.shape[0], x.shape[1], _p(y), _stream()))
    return y


def bias_tanh_bwd(y, gy):
    n, d = y.shape
    gx = torch.empty_like(y)
    parts = torch.empty((lib().oea_colsum_blocks(n), d), dtype=torch.float32, device=y.device)
    check(lib().oea_bias_tanh_bwd(_p(y), _p(gy), n, d, _p(gx), _p(parts), _stream()))
    return gx, parts.sum(0)


def segment_sum(vals, order, seg_ptr):
    """out[s] = sum of vals[order[e]] over e in [seg_ptr[s], seg_ptr[s + 1]) (order may be None) -> fp32 [n_seg]."""
    n_seg = seg_ptr.numel() - 1
    out = torch.empty(n_seg, dtype=torch.float32, device=vals.device)
    check(lib().oea_segment_sum_f32(_p(vals), _p(order), _p(seg_ptr), n_seg, _p(out), _stream()))
    return out
