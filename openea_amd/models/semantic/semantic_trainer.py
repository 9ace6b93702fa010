"""The trainer of HolE, SimplE and DistMult: one optimiser instance over the entity and relation tables (generate_optimizer,
hole.py:85-86 / simple.py:86-88 / distmult.py:59), stepped by oea_semantic_step (csrc/semantic_step.hip)."""
import torch

from ... import ops


class SemanticTrainer:
    """Same interface as TripleTrainer (step / pop_loss / dist) without the fused epoch call: RelationTripleEpochs drives it
    step by step with the (pos, neg) batches of the device sampler."""
    fused_epoch = False

    def __init__(self, model, ent, rel, cfg, optimizer):
        if optimizer not in ('Adagrad', 'SGD'):
            raise NotImplementedError("HolE / SimplE / DistMult: optimizer=%s -- the semantic step trains with Adagrad (the shipped args "
                                      "files) or SGD" % optimizer)
        self.model, self.ent, self.rel, self.cfg = model, ent, rel, cfg
        dev = ent.var.device
        if optimizer == 'Adagrad':        # tf.train.AdagradOptimizer: initial_accumulator_value = 0.1
            self.ent_acc = torch.full_like(ent.var, 0.1)
            self.rel_acc = torch.full_like(rel.var, 0.1)
        else:
            self.ent_acc = self.rel_acc = None
        self.ws = ops.step_workspace(ent.rows, rel.rows, ent.ld, dev)
        self.loss = torch.zeros(1, dtype=torch.float64, device=dev)
        self.dist = None
        self.t = 0

    def step(self, pos, neg):
        """pos: device int32 [n, 3]; neg: [n * k, 3], neg[p*k:(p+1)*k] the corruptions of pos p."""
        self.t += 1
        ops.semantic_step(self.model, self.ent.var, self.ent_acc, self.rel.var, self.rel_acc, self.ent.dim, pos, neg, self.cfg,
                          self.ws, self.loss)

    def pop_loss(self):
        v = float(self.loss.item())
        self.loss.zero_()
        return v


def check_device_path(model):
    """the limits of the semantic step, raised before any table is made"""
    name = type(model).__name__
    if model._dist_group() is not None:
        raise NotImplementedError("%s runs on one GPU: the data-parallel exchange of the semantic step is not built (launch it "
                                  "without torch.distributed, or with one rank)" % name)
    if model.args.dim > ops.SEMANTIC_MAX_DIM:
        raise NotImplementedError("%s: dim %d > %d (the semantic step holds a row in two columns per lane of one wave)"
                                  % (name, model.args.dim, ops.SEMANTIC_MAX_DIM))


def check_args(model, required):
    a = model.args
    for key, value in required.items():
        assert getattr(a, key) == value, "%s: %s must be %r" % (type(model).__name__, key, value)
