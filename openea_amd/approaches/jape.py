"""JAPE (mirror of openea/approaches/jape.py:18-169): Attr2Vec's attribute embeddings give a similarity matrix between the
reference (valid + test) entities of the two KGs; the joint training is a triple loss without a hinge,
    sum_pos |h + r - t|^2 - neg_alpha sum_neg |h + r - t|^2          (jape.py:74-84; oea_jape_step, csrc/jape_step.hip)
followed every epoch by the similarity loss beta |ref1 - l2n(sim[idx, :] @ ref2)|^2 over n_ref1 // sub_mat_size sampled blocks.

Two facts of the reference are kept as they are:
  * launch_sim_1epo fetches ONLY self.sim_loss (jape.py:136): sim_optimizer is built (jape.py:97) and never run, so the similarity
    loss is printed every epoch and trains nothing.  Here it is computed (oea_jape_sim_loss, csrc/sim_csr.hip) and printed, and no
    variable is updated there.  Training on it is out of scope.
  * after `sim_mat[sim_mat < attr_sim_mat_threshold] = 0` (jape.py:148) the matrix is sparse: it is held as a CSR
    (Attr2Vec.eval_sim_csr) instead of the reference's dense [n_ref, n_ref] fp32 array, 25.6 GB at the 100K split."""
import math
import time

import numpy as np
import torch

from .. import ops
from ..models.basic_model import BasicModel
from ..modules.finding.evaluation import early_stop
from ..modules.utils.util import task_divide
from .attr2vec import Attr2Vec


class JapeTrainer:
    """The interface of SemanticTrainer (step / pop_loss, no fused epoch call): RelationTripleEpochs drives it step by step with
    the (pos, neg) batches of the device sampler's uniform negatives."""
    fused_epoch = False

    def __init__(self, ent, rel, cfg, optimizer, neg_alpha):
        if optimizer not in ('Adagrad', 'SGD'):
            raise NotImplementedError("JAPE: optimizer=%s -- the triple step trains with Adagrad (the shipped args files) or SGD"
                                      % optimizer)
        self.ent, self.rel, self.cfg, self.neg_alpha = ent, rel, cfg, float(neg_alpha)
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
        ops.jape_step(self.ent.var, self.ent_acc, self.rel.var, self.rel_acc, self.ent.dim, pos, neg, self.neg_alpha, self.cfg,
                      self.ws, self.loss)

    def pop_loss(self):
        v = float(self.loss.item())
        self.loss.zero_()
        return v


class JAPE(BasicModel):

    def __init__(self):
        super().__init__()
        self.attr2vec = Attr2Vec()
        self.attr_sim_mat = None
        self.ref_entities1, self.ref_entities2 = None, None

    def init(self):
        self._check_args()
        self._check_device_path()
        self.ref_entities1 = self.kgs.valid_entities1 + self.kgs.test_entities1
        self.ref_entities2 = self.kgs.valid_entities2 + self.kgs.test_entities2
        self._define_variables()
        self._define_embed_graph()
        self._define_sim_graph()

    def _check_args(self):
        # customize parameters (jape.py:35-50)
        assert self.args.alignment_module == 'sharing'
        assert self.args.init == 'normal'
        assert self.args.neg_sampling == 'uniform'
        assert self.args.optimizer == 'Adagrad'
        assert self.args.eval_metric == 'inner'
        assert self.args.loss_norm == 'L2'

        assert self.args.ent_l2_norm is True
        assert self.args.rel_l2_norm is True

        assert self.args.neg_triple_num >= 1
        assert self.args.neg_alpha >= 0.0
        assert self.args.top_attr_threshold > 0.0
        assert self.args.attr_sim_mat_threshold > 0.0
        assert self.args.attr_sim_mat_beta > 0.0

    def _check_device_path(self):
        """the limits of the two steps, raised before any table is made"""
        if self._dist_group() is not None:
            raise NotImplementedError("JAPE runs on one GPU: the data-parallel exchange of its triple step is not built (launch it "
                                      "without torch.distributed, or with one rank)")
        if self.args.dim > ops.JAPE_MAX_DIM:
            raise NotImplementedError("JAPE: dim %d > %d (the triple step holds a row in two columns per lane of one wave)"
                                      % (self.args.dim, ops.JAPE_MAX_DIM))

    def _define_embed_graph(self):
        """jape.py:59-84"""
        a = self.args
        self.triple_loss = "sum_pos |h + r - t|^2 - neg_alpha sum_neg |h + r - t|^2"
        cfg = ops.make_step_cfg(loss='margin-based', ent_l2_norm=self.ent_embeds.is_l2_norm, rel_l2_norm=self.rel_embeds.is_l2_norm,
                                optimizer=a.optimizer, lr=a.learning_rate, neg_group_k=a.neg_triple_num)
        self.triple_optimizer = cfg
        self._trainer = JapeTrainer(self.ent_embeds, self.rel_embeds, cfg, a.optimizer, a.neg_alpha)

    def _define_sim_graph(self):
        """jape.py:86-98.  sim_optimizer exists in the reference and is never run (jape.py:136): there is none here."""
        dev = self.ent_embeds.var.device
        self.sim_loss = "attr_sim_mat_beta sum |ref1 - l2n(attr_sim_mat[idx, :] @ ref2)|^2"
        self.sim_optimizer = None
        self._ref1_dev = ops.to_ids(np.asarray(self.ref_entities1, np.int32), dev)
        self._ref2_dev = ops.to_ids(np.asarray(self.ref_entities2, np.int32), dev)
        self._sim_loss_dev = torch.zeros(1, dtype=torch.float64, device=dev)
        self._sim_idx = torch.zeros(max(int(self.args.sub_mat_size), 1), dtype=torch.int32, device=dev)
        self._sim_step = 0

    def launch_sim_1epo(self, epoch):
        """jape.py:127-138: n_ref1 // sub_mat_size draws of sub_mat_size rows (random.sample = oea_sample_distinct), the loss of each
        added up and printed.  No variable changes."""
        t = time.time()
        n_ref, m = len(self.ref_entities1), int(self.args.sub_mat_size)
        steps = n_ref // m
        indptr, col, val = self.attr_sim_mat
        for _ in range(steps):
            idx = ops.sample_distinct(n_ref, m, self._seed + 1, self._sim_step, out=self._sim_idx)
            self._sim_step += 1
            ops.jape_sim_loss(self.ent_embeds.var, self.args.dim, self._ref1_dev, self._ref2_dev, indptr, col, val, idx,
                              self.args.attr_sim_mat_beta, self._sim_loss_dev)
        loss = float(self._sim_loss_dev.item())
        self._sim_loss_dev.zero_()
        print('epoch {}, sim loss: {:.4f}, cost time: {:.4f}s'.format(epoch, loss, time.time() - t))
        return loss

    def run_attr2vec(self):
        """jape.py:140-150; the thresholded matrix as a CSR"""
        t = time.time()
        print("Training attribute embeddings:")
        self.attr2vec.set_args(self.args)
        self.attr2vec.set_kgs(self.kgs)
        self.attr2vec._seed = self._seed
        self.attr2vec.init()
        self.attr2vec.run()
        self.attr_sim_mat = self.attr2vec.eval_sim_csr(self.args.attr_sim_mat_threshold)
        print("Training attributes ends. Total time = {:.3f} s.".format(time.time() - t))

    def run(self):
        """jape.py:152-169"""
        self.run_attr2vec()
        print("Joint training:")
        t = time.time()
        triples_num = self.kgs.kg1.relation_triples_num + self.kgs.kg2.relation_triples_num
        triple_steps = int(math.ceil(triples_num / self.args.batch_size))
        steps_tasks = task_divide(list(range(triple_steps)), self.args.batch_threads_num)
        for i in range(1, self.args.max_epoch + 1):
            self.launch_triple_training_1epo(i, triple_steps, steps_tasks, None, None, None)
            self.launch_sim_1epo(i)
            if i >= self.args.start_valid and i % self.args.eval_freq == 0:
                flag = self.valid(self.args.stop_metric)
                self.flag1, self.flag2, self.early_stop = early_stop(self.flag1, self.flag2, flag)
                if self.early_stop or i == self.args.max_epoch:
                    break
        if self._epochs is not None:
            self._epochs.check()
        print("Training ends. Total time = {:.3f} s.".format(time.time() - t))
