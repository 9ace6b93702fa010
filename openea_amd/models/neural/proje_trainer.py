"""The trainer of ProjE: one Adam instance over the eight variables (generate_optimizer, proje.py:73-74), the log-uniform
candidate sampler stepped by (seed, global step) and oea_proje_step (csrc/proje_step.hip)."""
import torch

from ... import ops


class ProjETrainer:
    """Same interface as SemanticTrainer (step / pop_loss / dist): RelationTripleEpochs drives it step by step with the
    positive batches; there are no negative triples."""
    fused_epoch = False

    def __init__(self, variables, dim, n_sampled, lr, max_pos, seed=0):
        """variables: the eight device tensors in the order of ops.PROJE_VARS (the trainer updates them in place)"""
        self.variables = list(variables)
        ent, rel = self.variables[0], self.variables[1]
        dev = ent.device
        self.dim, self.lr = int(dim), float(lr)
        self.m = [torch.zeros_like(v) for v in self.variables]
        self.v = [torch.zeros_like(v) for v in self.variables]
        self.sampler = ops.LogUniformSampler(ent.shape[0], n_sampled, seed, dev)
        self.ws = ops.proje_workspace(ent.shape[0], rel.shape[0], self.dim, ent.shape[1], max_pos, n_sampled, dev)
        self.loss = torch.zeros(1, dtype=torch.float64, device=dev)
        self.dist = None
        self.t = 0

    def step(self, pos, neg=None):
        """pos: device int32 [n, 3] (the batches come from the model's own triples: their ids are not checked again)"""
        ids, num_tries, log_q = self.sampler.sample(self.t)
        self.t += 1
        ops.proje_step(self.variables, self.m, self.v, self.dim, pos, ids, log_q, num_tries, self.t, self.lr, self.ws, self.loss,
                       check_ids=False)

    def pop_loss(self):
        v = float(self.loss.item())
        self.loss.zero_()
        return v


def check_device_path(model):
    """the limits of the ProjE step, raised before any table is made"""
    name = type(model).__name__
    if model._dist_group() is not None:
        raise NotImplementedError("%s runs on one GPU: the data-parallel exchange of the ProjE step is not built (launch it "
                                  "without torch.distributed, or with one rank)" % name)
    if model.args.dim > ops.PROJE_MAX_DIM:
        raise NotImplementedError("%s: dim %d > %d (the ProjE step stages a row in a 128-column operand tile)"
                                  % (name, model.args.dim, ops.PROJE_MAX_DIM))
