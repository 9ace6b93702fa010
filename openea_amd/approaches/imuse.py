"""IMUSE (mirror of openea/approaches/imuse.py:17-345): before training, an interactive model aligns attributes by the similarity
of their names and then entities by the similarity of the values they hold under the aligned attributes; training is TransE's
margin loss under SGD plus a squared-distance pull on the entity pairs found.

All of the reference's run time is in `interactive_model`: for every entity of KG1 it walks every entity of KG2 and averages
Levenshtein.ratio over the aligned attribute pairs both hold (imuse.py:42-66), in eight Python processes.  Here the ratios are
computed on the device (csrc/lcs_sim.hip: ratio = 2 LCS / (|a| + |b|) over code points, LCS by a bit-vector recurrence) and the
n1 x n2 matrix never exists: oea_attr_sim_records returns, per KG1 entity, the RECORDS of its walk -- the (KG2 entity, similarity)
at which the similarity exceeds the threshold and every earlier one of the row.  run_one_ea's target_ent changes only there, so
the rest of the reference's logic (eight chunks, a fresh target_ent_set per chunk, union, dict) runs on the host over a dozen
records per entity, with the reference's own set and dict operations in the reference's order.

Deliberate differences:
  * ORDER.  The reference iterates sets that hold strings (kg.attribute_triples_set), so its result changes with PYTHONHASHSEED.
    Here filter_by_aligned_attributes walks kg.local_attribute_triples_list (sorted), the attribute ids walk in ascending order,
    and the aligned attribute pairs are a LIST in the order the name step produced them (by triple count, descending; ties in the
    order found) -- that list order is also the order in which a pair's ratios are added in fp64.
  * interactive_model_iter_num > 1 is refused.  The shipped args files have 1, so align_attribute_by_entities never runs there;
    and imuse.py:130-133 hands a set of ENTITY ids to filter_by_aligned_attributes, which compares it with ATTRIBUTE ids, so the
    second round computes nothing meaningful in the reference.
  * the commented-out cal_lcs_sim mix (imuse.py:181-198) is not built.
As in the reference, every alignment "batch" is the whole pair set, repeated ceil(|pairs| / batch_size) times an epoch
(imuse.py:319-326)."""
import math
import pickle
import time

import numpy as np
import torch

from .. import ops
from ..models.basic_model import BasicModel
from ..modules.finding.evaluation import early_stop
from ..modules.utils.util import task_divide

IMUSE_MAX_DIM = 128


def interactive_model(kgs, args):
    """imuse.py:17-39 for interactive_model_iter_num == 1."""
    if int(args.interactive_model_iter_num) > 1:
        raise NotImplementedError(
            "IMUSE: interactive_model_iter_num > 1 is not built.  The shipped args files have 1, and the reference's second round "
            "(align_attribute_by_entities, imuse.py:125-153) passes a set of entity ids where filter_by_aligned_attributes expects "
            "attribute ids (imuse.py:130-133), so it computes nothing meaningful there")
    start = time.time()
    aligned_attr_pairs = get_aligned_attr_pair_by_name_similarity(kgs, 0.6)
    print('aligned_attr_pair_set:', len(aligned_attr_pairs))
    aligned_ent_pair_set_all = set()
    aligned_ent_pair_set_iter = align_entity_by_attributes(kgs, aligned_attr_pairs, args.sim_thresholds_ent)
    aligned_ent_pair_set_all |= aligned_ent_pair_set_iter
    print(1, 'len(aligned_ent_pair_set_all):', len(aligned_ent_pair_set_all), 'len(aligned_ent_pair_set_iter):',
          len(aligned_ent_pair_set_iter))
    print(time.time() - start)
    return aligned_ent_pair_set_all


def filter_by_aligned_attributes(attr_triples, attr_set):
    """imuse.py:156-166, literally; attr_triples is walked in the order given (the caller passes a sorted list)."""
    ent_attrs_dict, ent_attr_value_dict = {}, {}
    for (e, a, v) in attr_triples:
        if a in attr_set and (e, a) not in ent_attr_value_dict:
            ent_attr_value_dict[(e, a)] = v
            attrs = set()
            if e in ent_attrs_dict:
                attrs = ent_attrs_dict[e]
            attrs.add(a)
            ent_attrs_dict[e] = attrs
    return ent_attrs_dict, ent_attr_value_dict


def select_name_pairs(attrs1, attrs2, sim, sim_thresholds_attr, triples1, triples2, top_k=10):
    """The host half of imuse.py:210-249 over the name ratios sim [len(attrs1), len(attrs2)] (fp64): for every attribute of KG1 in
    order the first KG2 attribute with the largest ratio above the threshold, if nobody took it before; then the top_k pairs by
    the number of attribute triples of their two attributes -> a list, largest first (ties in the order found)."""
    aligned, attr2_set = [], set()
    for i, attr1 in enumerate(attrs1):
        target_attr = None
        sim_max = sim_thresholds_attr
        for j, attr2 in enumerate(attrs2):
            if sim[i, j] > sim_max:
                target_attr = attr2
                sim_max = sim[i, j]
        if target_attr is not None and target_attr not in attr2_set:
            aligned.append((attr1, target_attr))
            attr2_set.add(target_attr)
    attr_num_dict_1, attr_num_dict_2 = {}, {}
    for (_, a, _) in triples1:
        attr_num_dict_1[a] = attr_num_dict_1.get(a, 0) + 1
    for (_, a, _) in triples2:
        attr_num_dict_2[a] = attr_num_dict_2.get(a, 0) + 1
    attr_pair_num_dict = {}
    for (a1, a2) in aligned:
        attr_pair_num_dict[(a1, a2)] = attr_num_dict_1.get(a1, 0) + attr_num_dict_2.get(a2, 0)
    attr_pair_list = sorted(attr_pair_num_dict.items(), key=lambda d: d[1], reverse=True)
    return [a_pair for (a_pair, _) in attr_pair_list[:min(top_k, len(attr_pair_list))]]


def get_aligned_attr_pair_by_name_similarity(kgs, sim_thresholds_attr, top_k=10):
    """imuse.py:201-249: the |A1| x |A2| ratios of the attribute names (the last segment of the URI) in one oea_lcs_ratio_pairs
    call, the selection on the host.  -> list of (attribute of KG1, attribute of KG2)."""
    attrs1, attrs2 = sorted(kgs.kg1.attributes_set), sorted(kgs.kg2.attributes_set)
    if not attrs1 or not attrs2:
        return []
    id_attr_dict_1 = {i: a for a, i in kgs.kg1.attributes_id_dict.items()}
    id_attr_dict_2 = {i: a for a, i in kgs.kg2.attributes_id_dict.items()}
    names1 = [id_attr_dict_1[a].split('/')[-1] for a in attrs1]
    names2 = [id_attr_dict_2[a].split('/')[-1] for a in attrs2]
    pool1, pool2 = ops.StringPool(names1), ops.StringPool(names2)
    pairs = np.stack(np.meshgrid(pool1.ids(names1), pool2.ids(names2), indexing='ij'), -1).reshape(-1, 2)
    _, ratio = ops.lcs_ratio_pairs(pool1, pool2, ops.to_ids(pairs, pool1.cp.device))
    sim = ratio.cpu().numpy().reshape(len(attrs1), len(attrs2))
    return select_name_pairs(attrs1, attrs2, sim, sim_thresholds_attr, kgs.kg1.attribute_triples_list,
                             kgs.kg2.attribute_triples_list, top_k)


def value_tables(aligned_attr_pairs, triples1, triples2, dev=None):
    """What oea_attr_sim_records reads, from the reference's own dictionaries -> (ents1, ents2, pool1, pool2, idx1, idx2): the
    entities in the order of ent_attrs_dict's keys (imuse.py:78: that order is the walk), the two string pools, and idx int32
    [K, n] on the device = the value entity i holds for pair k, -1 for none."""
    tables = []
    for side, triples in ((0, triples1), (1, triples2)):
        attrs = [p[side] for p in aligned_attr_pairs]
        ent_attrs_dict, value_dict = filter_by_aligned_attributes(triples, set(attrs))
        ents = list(ent_attrs_dict.keys())
        pool = ops.StringPool(value_dict.values(), dev)
        idx = np.full((len(attrs), max(len(ents), 1)), -1, np.int32)
        row = {e: i for i, e in enumerate(ents)}
        col = {a: k for k, a in enumerate(attrs)}
        for (e, a), v in value_dict.items():
            idx[col[a], row[e]] = pool.index[v]
        tables.append((ents, pool, idx))
    (ents1, pool1, idx1), (ents2, pool2, idx2) = tables
    return ents1, ents2, pool1, pool2, idx1, idx2


def select_entity_pairs(ents1, ents2, ptr, col):
    """imuse.py:78-97 over the records (ptr / col: ops.attr_sim_records): eight contiguous chunks of KG1's entities, the last one
    with the remainder; in a chunk run_one_ea's bookkeeping -- the target changes at a record, and it is taken if nobody of the
    chunk took it before; the union of the chunks in order; one pair per KG1 entity through dict().  The sets are built by the
    reference's operations in the reference's order (a chunk's set travels through pickle, as a pool result does), so that
    dict() keeps the same survivor."""
    aligned_ent_pair_set = set()
    size = len(ents1) // 8
    for i in range(8):
        lo, hi = size * i, (len(ents1) if i == 7 else size * (i + 1))
        aligned_ent_pair_set_i, target_ent_set = set(), set()
        for r in range(lo, hi):
            for j in col[ptr[r]:ptr[r + 1]]:
                target_ent = ents2[j]
                if target_ent not in target_ent_set:
                    aligned_ent_pair_set_i.add((ents1[r], target_ent))
                    target_ent_set.add(target_ent)
        aligned_ent_pair_set |= pickle.loads(pickle.dumps(aligned_ent_pair_set_i))
    temp_dict = dict([(x, y) for (x, y) in aligned_ent_pair_set])
    return set([(x, y) for x, y in temp_dict.items()])


def align_entity_by_attributes(kgs, aligned_attr_pairs, sim_thresholds_ent):
    """imuse.py:69-97: the records on the device, the selection on the host."""
    print('align_entity_by_attributes...')
    if len(aligned_attr_pairs) == 0:
        return set()
    ents1, ents2, pool1, pool2, idx1, idx2 = value_tables(aligned_attr_pairs, kgs.kg1.local_attribute_triples_list,
                                                          kgs.kg2.local_attribute_triples_list)
    if not ents1 or not ents2:
        return set()
    dev = pool1.cp.device
    ptr, col, _ = ops.attr_sim_records(pool1, pool2, ops.to_ids(idx1, dev), ops.to_ids(idx2, dev), sim_thresholds_ent)
    return select_entity_pairs(ents1, ents2, ptr, col)


class IMUSE(BasicModel):

    def __init__(self):
        super().__init__()
        self.aligned_ent_pair_set = None

    def init(self):
        self._check_args()
        if self._dist_group() is not None:
            raise NotImplementedError("IMUSE runs on one GPU (launch it without torch.distributed, or with one rank)")
        if self.args.dim > IMUSE_MAX_DIM:
            raise NotImplementedError("IMUSE: dim %d > %d" % (self.args.dim, IMUSE_MAX_DIM))
        ops.lib()
        self.aligned_ent_pair_set = interactive_model(self.kgs, self.args)
        self._define_variables()
        self._define_embed_graph()
        self._define_align_graph()

    def _check_args(self):
        # customize parameters (imuse.py:264-276)
        assert self.args.init == 'normal'
        assert self.args.loss == 'margin-based'
        assert self.args.neg_sampling == 'uniform'
        assert self.args.optimizer == 'SGD'
        assert self.args.eval_metric == 'inner'
        assert self.args.loss_norm == 'L2'

        assert self.args.ent_l2_norm is True
        assert self.args.rel_l2_norm is True

        assert self.args.neg_triple_num == 1
        assert self.args.learning_rate >= 0.01

    def _define_align_graph(self):
        """imuse.py:304-313: align_loss = sum |e1 - e2|^2 over the normalised rows of the pairs, plain SGD on the variable.  The pair
        set never changes, so its endpoints are grouped by row once."""
        self.align_loss = "sum |l2n(ent)[e1] - l2n(ent)[e2]|^2"
        self.align_optimizer = dict(optimizer='SGD', lr=self.args.learning_rate)
        dev = self.ent_embeds.var.device
        pairs = np.asarray(list(self.aligned_ent_pair_set), np.int32).reshape(-1, 2)
        self._align_pairs = ops.to_ids(pairs, dev)
        self._align_all = torch.arange(self.ent_embeds.rows, dtype=torch.int32, device=dev)
        self._align_csr = ops.pair_rows_csr(self._align_pairs, self.ent_embeds.rows) if len(pairs) else None

    def align_step(self):
        """One session.run([align_loss, align_optimizer]) (imuse.py:322) -> the loss as a device scalar.  T = l2_normalize(ent);
        d loss / d T by rows without atomics (oea_pair_grad_rows over the row-grouped endpoints, coefficient 1 per pair);
        ent -= lr * (that gradient pulled back through the normalisation) (oea_sgd_rows)."""
        ent = self.ent_embeds
        t = ops.gather_rows(ent.var, ent.dim, self._align_all, normalize=ent.is_l2_norm, out_ld=ent.ld)
        terms, coef = ops.pair_loss_l2_fwd(t, ent.dim, self._align_pairs, self._align_pairs.shape[0], None, 0.0, 0.0)
        grad = ops.pair_grad_rows(t, ent.dim, *self._align_csr, coef, norm=2)
        ops.sgd_rows_(ent.var, grad, ent.dim, ent.is_l2_norm, self.args.learning_rate)
        return terms.sum(dtype=torch.float64)

    def launch_align_training_1epo(self, epoch):
        """imuse.py:315-328"""
        start = time.time()
        n_pairs = len(self.aligned_ent_pair_set)
        steps = int(math.ceil(n_pairs / self.args.batch_size))
        epoch_loss = torch.zeros((), dtype=torch.float64, device=self.ent_embeds.var.device)
        for _ in range(steps):
            epoch_loss += self.align_step()
        trained_samples_num = steps * n_pairs
        epoch_loss = float(epoch_loss.item()) / max(trained_samples_num, 1)          # no pair: no step, and a loss of 0
        print('epoch {}, align learning loss: {:.4f}, time: {:.4f}s'.format(epoch, epoch_loss, time.time() - start))
        return epoch_loss

    def run(self):
        """imuse.py:330-345"""
        t = time.time()
        relation_triples_num = len(self.kgs.kg1.relation_triples_list) + len(self.kgs.kg2.relation_triples_list)
        relation_triple_steps = int(math.ceil(relation_triples_num / self.args.batch_size))
        relation_step_tasks = task_divide(list(range(relation_triple_steps)), self.args.batch_threads_num)
        for i in range(1, self.args.max_epoch + 1):
            self.launch_triple_training_1epo(i, relation_triple_steps, relation_step_tasks, None, None, None)
            self.launch_align_training_1epo(i)
            if i >= self.args.start_valid and i % self.args.eval_freq == 0:
                flag = self.valid(self.args.stop_metric)
                self.flag1, self.flag2, self.early_stop = early_stop(self.flag1, self.flag2, flag)
                if self.early_stop or i == self.args.max_epoch:
                    break
        if self._epochs is not None:
            self._epochs.check()
        print("Training ends. Total time = {:.3f} s.".format(time.time() - t))
