"""The trainer of ConvE: one Adam instance over the fourteen variables (generate_optimizer, conve.py:78-79), ProjE's log-uniform
candidate sampler and oea_conve_step (csrc/conve_step.hip).  The global step drives both the sampler and the dropout masks."""
import torch

from ... import ops
from . import proje_trainer


class ConvETrainer:
    """ProjETrainer's interface (step / pop_loss / dist): RelationTripleEpochs drives it step by step with the positive
    batches; there are no negative triples."""
    fused_epoch = False

    def __init__(self, variables, dim, filters, keep_prob, n_sampled, lr, max_pos, seed=0):
        """variables: the fourteen device tensors in the order of ops.CONVE_VARS (the trainer updates them in place)"""
        self.variables = list(variables)
        ent, rel = self.variables[0], self.variables[1]
        dev = ent.device
        self.dim, self.filters, self.keep_prob, self.lr, self.seed = int(dim), int(filters), float(keep_prob), float(lr), int(seed)
        self.m = [torch.zeros_like(v) for v in self.variables]
        self.v = [torch.zeros_like(v) for v in self.variables]
        self.sampler = ops.LogUniformSampler(ent.shape[0], n_sampled, seed, dev)
        self.ws = ops.conve_workspace(ent.shape[0], rel.shape[0], self.dim, ent.shape[1], self.filters, max_pos, n_sampled, dev)
        self.loss = torch.zeros(1, dtype=torch.float64, device=dev)
        self.dist = None
        self.t = 0

    def step(self, pos, neg=None):
        """pos: device int32 [n, 3] (the batches come from the model's own triples: their ids are not checked again)"""
        ids, num_tries, log_q = self.sampler.sample(self.t)
        mask_step = self.t
        self.t += 1
        ops.conve_step(self.variables, self.m, self.v, self.dim, self.filters, self.keep_prob, self.seed, pos, ids, log_q, num_tries,
                       mask_step, self.t, self.lr, self.ws, self.loss, check_ids=False)

    def pop_loss(self):
        v = float(self.loss.item())
        self.loss.zero_()
        return v


def check_device_path(model):
    """the limits of the ConvE step, raised before any table is made: ProjE's (one GPU, dim) and the filter count"""
    proje_trainer.check_device_path(model)
    f = model.args.filter_num
    if not 1 <= f <= ops.CONVE_MAX_FILTERS:
        raise NotImplementedError("%s: filter_num %d outside [1, %d] (the ConvE step keeps a filter's gradients in fixed slots)"
                                  % (type(model).__name__, f, ops.CONVE_MAX_FILTERS))
