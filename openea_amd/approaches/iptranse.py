"""IPTransE (mirror of openea/approaches/iptranse.py:21-321): margin-based TransE pairs plus a loss on two-step relation paths,
both under one Adagrad instance, and every bp_freq epochs an alignment epoch -- greedy pairs of the reference (valid + test)
entities above sim_th, the triples with the aligned entity swapped in, and steps of the similarity-weighted margin loss under a
second, independent Adagrad instance.

The training step is the fused oea_ptranse_step (csrc/ptranse_step.hip): the step engine's margin kernel on the triples, the
path half through the Gram matrix of the normalised relation table, one optimiser pass on the summed gradient; an epoch is
enqueued by one call (oea_ptranse_epoch) after its negatives and path batches were drawn by one launch each.  The alignment
steps run oea_weighted_pair_step.

Where this differs from the reference on purpose: if both KGs have no two-step path the reference divides by zero
(iptranse.py:77); here the path half is skipped (P = 0: plain TransE steps) and one printed line says so."""
import math
import random
import time

import numpy as np
import torch

from .. import ops
from ..models.basic_model import BasicModel
from ..models.trainer import TripleTrainer
from ..modules.base.losses import margin_loss
from ..modules.bootstrapping.alignment_finder import PairSim, find_alignment_arrays
from ..modules.finding.evaluation import early_stop
from ..modules.load.kgs import KGs
from ..modules.utils.util import task_divide

MAX_PATH_WEIGHT = 101          # iptranse.py:106: paths with weight < 101 are kept


def generate_neg_paths(pos_paths, rel_list):
    """iptranse.py:21-26: (r_x, r_y, r') with r' one uniform draw from rel_list (it may equal r)."""
    return [(r_x, r_y, random.sample(rel_list, 1)[0]) for (r_x, r_y, _, _) in pos_paths]


def generate_newly_triples(ent1, ent2, w, rt_dict1, hr_dict1):
    """iptranse.py:29-35: ent1's triples with ent2 in its place, each carrying the weight w."""
    out = {(ent2, r, t, w) for r, t in rt_dict1.get(ent1, set())}
    out |= {(h, r, ent2, w) for h, r in hr_dict1.get(ent1, set())}
    return out


def generate_triples_of_latent_ents(kgs: KGs, ents1, ents2, tr_ws):
    """iptranse.py:38-45."""
    assert len(ents1) == len(ents2)
    newly_triples = set()
    for e1, e2, w in zip(ents1, ents2, tr_ws):
        newly_triples |= generate_newly_triples(e1, e2, w, kgs.kg1.rt_dict, kgs.kg1.hr_dict)
        newly_triples |= generate_newly_triples(e2, e1, w, kgs.kg2.rt_dict, kgs.kg2.hr_dict)
    print("newly triples: {}".format(len(newly_triples)))
    return newly_triples


def generate_neg_triples_w(pos_triples, ents_list):
    """iptranse.py:48-58: head with probability 1/2, else tail, replaced by a uniform draw from ents_list; the negative inherits
    the positive's weight."""
    neg_triples = []
    for (h, r, t, w) in pos_triples:
        if random.randint(0, 999) < 500:
            neg_triples.append((random.sample(ents_list, 1)[0], r, t, w))
        else:
            neg_triples.append((h, r, random.sample(ents_list, 1)[0], w))
    return neg_triples


def generate_triple_batch(triples, batch_size, ents_list):
    """iptranse.py:61-66: min(batch_size, len) distinct triples and one negative each."""
    triples = triples if isinstance(triples, (list, tuple)) else sorted(triples)
    pos_triples = random.sample(triples, min(batch_size, len(triples)))
    return pos_triples, generate_neg_triples_w(pos_triples, ents_list)


def _expand(lo, cnt):
    """indices lo[i] .. lo[i] + cnt[i] - 1 for every i, back to back, and the i of each -> (rep, idx)"""
    total = int(cnt.sum())
    rep = np.repeat(np.arange(len(cnt), dtype=np.int64), cnt)
    start = np.cumsum(cnt) - cnt
    return rep, lo[rep] + (np.arange(total, dtype=np.int64) - start[rep])


def two_step_path_arrays(triples):
    """generate_2steps_path as arrays: int64 [n, 3] = (r_x, r_y, r) and float64 [n] weights (order free)."""
    tr = np.asarray(triples, np.int64).reshape(-1, 3)
    if len(tr) == 0:
        return np.zeros((0, 3), np.int64), np.zeros(0, np.float64)
    h, r, t = tr[:, 0], tr[:, 1], tr[:, 2]
    n_e, n_r = int(max(h.max(), t.max())) + 1, int(r.max()) + 1
    _, inv, counts = np.unique(h * n_r + r, return_inverse=True, return_counts=True)
    size = counts[inv.reshape(-1)]                         # tails of the edge's (h, r) group (iptranse.py:98-100)
    # every group size is >= 1, so an edge whose group already has >= 101 tails can never be in a path of weight < 101
    keep = np.nonzero(size < MAX_PATH_WEIGHT)[0]
    kh, kt, ks = h[keep], t[keep], size[keep]
    order = np.argsort(kh, kind="stable")
    hs = kh[order]
    lo = np.searchsorted(hs, kt, "left")
    i1, j = _expand(lo, np.searchsorted(hs, kt, "right") - lo)      # (h, r1, m) x (m, r2, t)  (iptranse.py:102)
    i2 = order[j]
    w = ks[i1] * ks[i2]
    ok = w < MAX_PATH_WEIGHT                               # iptranse.py:105-106
    i1, i2, w = i1[ok], i2[ok], w[ok]
    # the closing triples (h, r, t) of ALL triples (iptranse.py:107)
    key = h * n_e + t
    korder = np.argsort(key, kind="stable")
    ksorted = key[korder]
    q = kh[i1] * n_e + kt[i2]
    lo = np.searchsorted(ksorted, q, "left")
    p, c = _expand(lo, np.searchsorted(ksorted, q, "right") - lo)
    paths = np.stack([r[keep][i1[p]], r[keep][i2[p]], r[korder[c]]], axis=1)
    return paths, w[p].astype(np.float64)


def generate_2steps_path(triples):
    """iptranse.py:95-115 in numpy (no pandas at run time): for triples (h, r1, m), (m, r2, t) and a closing triple (h, r, t) one
    (r1, r2, r, w) with w = #tails of (h, r1) x #tails of (m, r2), kept when w < 101.  The same multiset as the reference's
    pandas recipe returns, in another order.  Runs once per run on the host, where the triple lists live."""
    paths, w = two_step_path_arrays(triples)
    print("num of path:", paths.shape[0])
    return [(int(a), int(b), int(c), float(x)) for (a, b, c), x in zip(paths.tolist(), w.tolist())]


class IPTransE(BasicModel):

    def __init__(self):
        super().__init__()
        self.ref_entities1, self.ref_entities2 = None, None
        self.paths1, self.paths2 = None, None
        self._no_paths_said = False

    def init(self):
        """iptranse.py:125-149"""
        if self._dist_group() is not None:
            raise NotImplementedError("IPTransE runs on one GPU: the path half and the alignment steps add to the gradient scratch "
                                      "outside the partitioned step (launch it without torch.distributed, or with one rank)")
        self._check_args()
        self.ref_entities1 = self.kgs.valid_entities1 + self.kgs.test_entities1
        self.ref_entities2 = self.kgs.valid_entities2 + self.kgs.test_entities2
        self.paths1 = generate_2steps_path(self.kgs.kg1.relation_triples_list)
        self.paths2 = generate_2steps_path(self.kgs.kg2.relation_triples_list)
        self._define_variables()
        self._define_embed_graph()
        self._define_alignment_graph()

    def _check_args(self):
        # customize parameters (iptranse.py:136-149)
        assert self.args.alignment_module == 'sharing'
        assert self.args.init == 'normal'
        assert self.args.neg_sampling == 'uniform'
        assert self.args.optimizer == 'Adagrad'
        assert self.args.eval_metric == 'inner'
        assert self.args.loss_norm == 'L2'
        assert self.args.ent_l2_norm is True
        assert self.args.rel_l2_norm is True
        assert self.args.margin > 0.0
        assert self.args.neg_triple_num == 1
        assert self.args.sim_th > 0.0

    def _define_embed_graph(self):
        """iptranse.py:183-215: train_loss = margin pairs + path_parm * path loss under ONE optimiser instance."""
        self.train_loss = margin_loss(self.args.margin, self.args.loss_norm)
        cfg, opt = self._step_cfg(self.train_loss, 0)
        self.optimizer = cfg
        self._trainer = TripleTrainer(self.ent_embeds, self.rel_embeds, cfg, opt)
        dev = self.ent_embeds.var.device
        self._path_ws = ops.path_workspace(self.rel_embeds.rows, self.rel_embeds.ld, dev)
        self._path_dev = []
        for paths, kg in ((self.paths1, self.kgs.kg1), (self.paths2, self.kgs.kg2)):
            arr = np.asarray([p[:3] for p in paths], np.int32).reshape(-1, 3)
            w = np.asarray([p[3] for p in paths], np.float32)
            self._path_dev.append((ops.to_ids(arr, dev), ops.to_vec(w, dev), ops.to_ids(np.asarray(kg.relations_list, np.int32), dev)))
        self._path_batches = None

    def _define_alignment_graph(self):
        """iptranse.py:217-235: its own optimiser instance -> its own accumulators."""
        self.alignment_loss = margin_loss(self.args.margin, 'L2')
        cfg, opt = self._step_cfg(self.alignment_loss, 0)
        self.alignment_optimizer = cfg
        self._align_trainer = TripleTrainer(self.ent_embeds, self.rel_embeds, cfg, opt, replicated=True)

    def _ref_sim_mat(self):
        """iptranse.py:237-241: lookup(ref1) . lookup(ref2)^T, evaluated on demand on the device (no n x n host matrix)."""
        return PairSim(self.ent_embeds.lookup(self.ref_entities1), self.ent_embeds.lookup(self.ref_entities2), self.args.dim)

    def _path_batch_size(self, triple_steps):
        """iptranse.py:245; 0 (and one printed line) when neither KG has a two-step path."""
        n = len(self.paths1) + len(self.paths2)
        if n == 0:
            if not self._no_paths_said:
                print("IPTransE: no two-step relation path in either KG -- the path loss is skipped (plain TransE steps)")
                self._no_paths_said = True
            return 0
        return n // triple_steps

    def launch_ptranse_training_1epo(self, epoch, triple_steps, steps_tasks, batch_queue):
        """iptranse.py:243-272.  `steps_tasks` / `batch_queue` belonged to the host producers and are ignored."""
        start = time.time()
        ep = self._ensure_epochs(True)
        b = ep.batches
        steps = len(b.splits)
        path_batch_size = self._path_batch_size(steps)
        if ep._sides is None:
            ep._sides = (ep.s1.side(), ep.s2.side())
        neg_all = ep._epoch_neg_buf()
        ops.sample_negatives_epoch(b.dall, ep._off_dev, ep._spl_dev, steps, ep.k, ep._sides[0], ep._sides[1], ep.seed, ep._epoch_base,
                                   neg_all, ep.err)
        if path_batch_size > 0:
            (p1, w1, r1), (p2, w2, r2) = self._path_dev
            self._path_batches = ops.path_sample_epoch(p1, w1, p2, w2, r1, r2, steps, self._seed, epoch, out=self._path_batches)
        t = self._trainer
        t.count_steps(steps)
        ops.ptranse_epoch(self.ent_embeds.var, t.ent_acc, self.rel_embeds.var, t.rel_acc, self.args.dim, b.dall, b.offsets, neg_all,
                          self._path_batches if path_batch_size > 0 else None, float(self.args.path_parm), t.cfg, t.ws, self._path_ws,
                          t.loss, check_ids=False)
        ep.global_step += steps
        ep._epoch_base = ep.global_step
        epoch_loss = t.pop_loss()                       # the one host read of the epoch
        ops.path_check(self._path_ws[1])
        epoch_loss /= self.args.batch_size              # iptranse.py:269
        b.shuffle(ep.gen)                               # iptranse.py:270-271
        print('epoch {}, avg. triple loss: {:.4f}, cost time: {:.4f}s'.format(epoch, epoch_loss, time.time() - start))

    def launch_alignment_training_1epo(self, epoch):
        """iptranse.py:274-303; the batch draw and the corruption of every step run on the device with torch's generator."""
        t1 = time.time()
        sim = self._ref_sim_mat()
        found = find_alignment_arrays(sim, self.args.sim_th, 1)
        if found is None or len(found[0]) == 0:
            return
        ii, jj, ws = found
        new_ent1 = [self.ref_entities1[i] for i in ii.tolist()]
        new_ent2 = [self.ref_entities2[j] for j in jj.tolist()]
        newly_triples = generate_triples_of_latent_ents(self.kgs, new_ent1, new_ent2, [float(w) for w in ws.tolist()])
        if len(newly_triples) == 0:
            return
        steps = max(math.ceil(len(newly_triples) / self.args.batch_size), 1)
        dev = self.ent_embeds.var.device
        rows = sorted(newly_triples)
        tri = ops.to_ids(np.asarray([x[:3] for x in rows], np.int32), dev)
        w_dev = ops.to_vec(np.asarray([x[3] for x in rows], np.float32), dev)
        ents = ops.to_ids(np.asarray(self.kgs.kg1.entities_list + self.kgs.kg2.entities_list, np.int32), dev)
        n, n_batch = tri.shape[0], min(self.args.batch_size, tri.shape[0])
        gen = torch.Generator(device=dev)
        gen.manual_seed(self._seed + 2000 + epoch)
        picks = torch.rand((steps, n), device=dev, generator=gen).argsort(dim=1)[:, :n_batch]
        head = torch.rand((steps, n_batch), device=dev, generator=gen) < 0.5
        repl = ents[torch.randint(0, ents.numel(), (steps, n_batch), device=dev, generator=gen)]
        t = self._align_trainer
        for step in range(steps):
            pos = tri[picks[step]].contiguous()
            neg = pos.clone()
            neg[:, 0] = torch.where(head[step], repl[step], pos[:, 0])
            neg[:, 2] = torch.where(head[step], pos[:, 2], repl[step])
            t.count_steps()
            ops.weighted_pair_step(self.ent_embeds.var, t.ent_acc, self.rel_embeds.var, t.rel_acc, self.args.dim, pos, neg,
                                   w_dev[picks[step]].contiguous(), t.cfg, t.ws, t.loss)
        alignment_loss = t.pop_loss() / len(newly_triples)
        print('epoch {}, alignment loss: {:.4f}, cost time: {:.4f}s'.format(epoch, alignment_loss, time.time() - t1))

    def run(self):
        """iptranse.py:305-321 (range(1, max_epoch): the last epoch is max_epoch - 1; the alignment epoch follows the validation)"""
        t = time.time()
        triples_num = self.kgs.kg1.relation_triples_num + self.kgs.kg2.relation_triples_num
        triple_steps = int(math.ceil(triples_num / self.args.batch_size))
        steps_tasks = task_divide(list(range(triple_steps)), self.args.batch_threads_num)
        for epoch in range(1, self.args.max_epoch):
            self.launch_ptranse_training_1epo(epoch, triple_steps, steps_tasks, None)
            if epoch >= self.args.start_valid and epoch % self.args.eval_freq == 0:
                flag = self.valid(self.args.stop_metric)
                self.flag1, self.flag2, self.early_stop = early_stop(self.flag1, self.flag2, flag)
                if self.early_stop or epoch == self.args.max_epoch:
                    break
            if epoch % self.args.bp_freq == 0:
                self.launch_alignment_training_1epo(epoch)
        if self._epochs is not None:
            self._epochs.check()
        print("Training ends. Total time = {:.3f} s.".format(time.time() - t))
