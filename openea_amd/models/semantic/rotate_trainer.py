"""What BootEA_RotatE (approaches/bootea_rotate.py) and the plain RotatE (models/semantic/rotate.py) share: the stacked fp64
entity table, the phase table and the trainer around oea_rotate_step (csrc/rotate_step.hip)."""
import numpy as np
import torch

from ... import ops


class ComplexEntityTable:
    """re_ent_embeds and im_ent_embeds (bootea_rotate.py:50-55) stacked in one fp64 device array [2E, ld]: rows [0, E)
    real parts, [E, 2E) imaginary parts.  `lookup` is what every consumer outside the training step reads: the sum
    of the two (row-normalised) parts as an fp32 block."""

    def __init__(self, re_host, im_host, is_l2_norm, dev=None):
        self.rows, self.dim = re_host.shape                      # E, d
        self.is_l2_norm = bool(is_l2_norm)
        self.var = ops.to_table64(np.concatenate([re_host, im_host]).astype(np.float64), dev)
        self.ld = self.var.shape[1]

    def _ids(self, ids):
        if ids is None or hasattr(ids, "is_cuda"):
            return ids
        return ops.to_ids(np.asarray(ids, np.int32), self.var.device)

    def lookup(self, ids, sum_norm=None):
        """l2n?(re)[ids] + l2n?(im)[ids], normalised again when sum_norm (default: the l2_norm flag, as
        eval_kg*_useful_ent_embeddings does, bootea_rotate.py:128-140) -> device fp32 [n, pad4(dim)]."""
        sum_norm = self.is_l2_norm if sum_norm is None else sum_norm
        return ops.rotate_lookup(self.var, self.dim, self._ids(ids), self.is_l2_norm, sum_norm)

    def parts(self):
        """host fp64 (re, im), each [E, dim], normalised when the flag is set: `re_ent_embeds.eval()`."""
        v = self.var[:, :self.dim].cpu().numpy()
        if self.is_l2_norm:
            v = v / np.sqrt(np.maximum((v * v).sum(1, keepdims=True), 1e-12))
        return v[:self.rows], v[self.rows:]


class PhaseTable:
    """rel_embeds (bootea_rotate.py:56-57): fp64 [R, ld] phases (before the pi / embedding_range scaling)."""

    def __init__(self, host, is_l2_norm, dev=None):
        self.rows, self.dim = host.shape
        self.is_l2_norm = bool(is_l2_norm)
        self.var = ops.to_table64(host.astype(np.float64), dev)

    def eval(self, session=None):
        v = self.var[:, :self.dim].cpu().numpy()
        if self.is_l2_norm:
            v = v / np.sqrt(np.maximum((v * v).sum(1, keepdims=True), 1e-12))
        return v


class RotateTrainer:
    """One optimiser instance over the three variables (generate_optimizer, bootea_rotate.py:107-109 / 156-158): its own
    Adam moments and step count.  neg_loss_div = k > 1 divides the negatives' half of the loss by k (the plain RotatE,
    rotate.py:81); BootEA_RotatE leaves it at 0.  Same interface as TripleTrainer (step / pop_loss / dist), without the fused epoch
    call: RelationTripleEpochs drives it step by step."""
    fused_epoch = False

    def __init__(self, ent, rel, args, neg_group_k, dist_group=None, replicated=False, neg_loss_div=0):
        self.ent, self.rel, self.k = ent, rel, int(neg_group_k)
        self.optimizer = args.optimizer
        self.cfg = ops.make_rotate_cfg(args.gamma, args.dim, ent.is_l2_norm, rel.is_l2_norm, args.optimizer, args.learning_rate,
                                       neg_loss_div=neg_loss_div)
        self.ent_state = ops.rotate_state(ent.var, args.optimizer)
        self.rel_state = ops.rotate_state(rel.var, args.optimizer)
        dev = ent.var.device
        self.ws = ops.rotate_workspace(ent.rows, rel.rows, ent.ld, dev)
        self.loss = torch.zeros(1, dtype=torch.float64, device=dev)
        self.t = 0
        self.dist, self.replicated = dist_group, bool(replicated)
        self.xchg = ops.rotate_exchange_view(self.ws, ent.rows, rel.rows, ent.ld) if dist_group is not None else None

    def _run(self, pos, neg, phase):
        ops.rotate_step(self.ent.var, self.ent_state, self.rel.var, self.rel_state, self.ent.dim, pos, neg,
                        self.k if neg is not None else 0, self.cfg, self.ws, self.loss, phase=phase)

    def step(self, pos, neg):
        self.t += 1
        self.cfg.t = self.t
        if self.dist is None:
            return self._run(pos, neg, ops.PHASE_BOTH)
        import torch.distributed as dist
        self._run(pos, neg, ops.PHASE_GRAD)
        dist.all_reduce(self.xchg, op=dist.ReduceOp.SUM, group=self.dist)
        if self.replicated:
            self.xchg /= dist.get_world_size(self.dist)
        self._run(pos, neg, ops.PHASE_APPLY)

    def pop_loss(self):
        if self.dist is not None and not self.replicated:
            import torch.distributed as dist
            dist.all_reduce(self.loss, op=dist.ReduceOp.SUM, group=self.dist)
        v = float(self.loss.item())
        self.loss.zero_()
        return v
