"""AttrE (mirror of openea/approaches/attre.py:19-257): TransE on the relation triples, a second translational model on the attribute
triples (e, a, v) whose value vector is composed from the first `literal_len` characters of the value,
    v = sum_p w_p char[id_p],   w_p = sum_{m = p + 1 .. L} 1 / m          (attre.py:88-109: the sum of the means of the prefixes),
and a joint loss sum_e (1 - ent_embeds[e] . ent_embeds_ce[e]) that pulls the two entity tables together.  An epoch is a relation
epoch (the engine every translational model here runs on), a character epoch (oea_attre_sample_heads + oea_attre_char_step,
csrc/attre_step.hip) and a joint epoch (oea_attre_joint_epoch: its ceil(E / batch_size) steps over ALL entities in one pass).

Deliberate differences:
  * CHARACTER IDS.  The reference numbers the kept characters in `list(set)` order, which changes with PYTHONHASHSEED.  Here they
    are numbered by descending count, then code point.  Id 0 (padding, and every dropped character) is a trained row as there.
  * SHUFFLE.  The reference trains its first epoch on the lists as loaded and shuffles them after every epoch; here every epoch
    draws a fresh keyed permutation of the lists as loaded (oea_epoch_layout), the distribution of shuffling the last order.
  * NEGATIVES.  Every attribute triple has a value id of its own, so the reference's redraw `while (e', a, v) in triples` rejects
    exactly e' == e: the device sampler draws uniformly over the other entities of the side's list, without a loop.
As in the reference every character batch is full (b1 + b2 = batch_size: a short last slice is topped up from the head of its
list, batch.py:48-57) -- the composition is not normalised and `batch_size` shapes its zeros, so a short batch would not even
broadcast there."""
import math
import time

import numpy as np
import torch

from .. import ops
from ..models.basic_model import BasicModel
from ..modules.base.initializers import init_embeddings
from ..modules.finding.evaluation import early_stop
from ..modules.utils.util import task_divide

CHAR_SHARE = 0.0001            # attre.py:52: a character is kept when its share of all characters reaches this


def clean_value(v):
    """attre.py:27-34"""
    v = v.split('(')[0].rstrip(' ')
    return v.replace('.', '').replace('(', '').replace(')', '').replace(',', '').replace('_', ' ').replace('-', ' ').split('"')[0]


def kept_characters(values):
    """attre.py:39-53 over the DISTINCT cleaned values -> the kept characters, by descending count, then code point (their ids are
    1 + the position here)"""
    counts = {}
    for literal in set(values):
        for ch in literal:
            counts[ch] = counts.get(ch, 0) + 1
    total = sum(counts.values())
    ranked = sorted(counts.items(), key=lambda kv: (-kv[1], ord(kv[0])))
    return [ch for ch, n in ranked if n / total >= CHAR_SHARE]


def formatting_attr_triples(kgs, literal_len):
    """attre.py:19-79 -> (attribute triples of KG1, of KG2 as (e, a, value id) lists, value_id_char_ids int32 [T1 + T2, literal_len],
    char_list_size).  Every triple gets a value id of its own, so a triple is (e, a, its own index).  The character ids follow
    kept_characters' order (descending count, then code point), not the reference's hash-seed dependent `list(set)`."""
    list1 = [(e, a, clean_value(v)) for (e, a, v) in kgs.kg1.local_attribute_triples_list]
    list2 = [(e, a, clean_value(v)) for (e, a, v) in kgs.kg2.local_attribute_triples_list]
    chars = kept_characters([v for (_, _, v) in list1 + list2])
    char_id = {ch: i + 1 for i, ch in enumerate(chars)}
    ids = np.zeros((len(list1) + len(list2), literal_len), np.int32)
    for row, (_, _, v) in enumerate(list1 + list2):
        for i, ch in enumerate(v[:literal_len]):
            ids[row, i] = char_id.get(ch, 0)
    new1 = [(e, a, i) for i, (e, a, _) in enumerate(list1)]
    new2 = [(e, a, len(list1) + i) for i, (e, a, _) in enumerate(list2)]
    return new1, new2, ids, len(chars) + 1


def attr_batch_layout(n1, n2, batch_size):
    """generate_attribute_triple_batch with is_fixed_size = True (batch.py:48-57, 214-225) as a gather map -> (slot int64 [steps *
    batch_size], b1, steps): step s reads slot[s * batch_size : (s + 1) * batch_size] of cat(list1, list2), its first b1 rows
    from KG1.  A short slice is topped up from the head of its list; a side that cannot fill its share raises ValueError."""
    if n1 + n2 < 1 or batch_size < 1:
        raise ValueError("attr_batch_layout: no attribute triples or no batch")
    b1 = int(n1 / (n1 + n2) * batch_size)
    b2 = batch_size - b1
    if b1 > n1 or b2 > n2:
        raise ValueError("AttrE: batch_size %d asks for %d + %d attribute triples a step of lists of %d + %d: the reference's "
                         "fixed-size batches (batch.py:55-56) cannot be filled" % (batch_size, b1, b2, n1, n2))
    steps = int(math.ceil((n1 + n2) / batch_size))
    slot = np.empty((steps, batch_size), np.int64)
    for s in range(steps):
        for off, b, n, base in ((0, b1, n1, 0), (b1, b2, n2, n1)):
            own = np.arange(min(s * b, n), min(s * b + b, n))
            slot[s, off:off + b] = np.concatenate([own, np.arange(b - len(own))]) + base
    return slot.reshape(-1), b1, steps


class AttrE(BasicModel):

    def __init__(self):
        super().__init__()
        self.ent_embeds_ce = self.attr_embeds = self.char_embeds = None
        self.char_path = ops.ATTRE_PATH_AUTO

    def init(self):
        self._check_device_path()
        self.attribute_triples_list1, self.attribute_triples_list2, self.value_id_char_ids, self.char_list_size = \
            formatting_attr_triples(self.kgs, self.args.literal_len)
        self._define_variables()
        self._define_embed_graph()

    def _check_device_path(self):
        """the limits of the steps, raised before any table is made"""
        a = self.args
        if self._dist_group() is not None:
            raise NotImplementedError("AttrE runs on one GPU: the exchange of its character and joint steps is not built (launch it "
                                      "without torch.distributed, or with one rank)")
        if a.dim > ops.ATTRE_MAX_DIM:
            raise NotImplementedError("AttrE: dim %d > %d (the character step holds a row in two columns per lane of one wave)"
                                      % (a.dim, ops.ATTRE_MAX_DIM))
        if a.optimizer not in ('SGD', 'Adagrad'):
            raise NotImplementedError("AttrE: optimizer=%s -- the character and joint steps train with SGD (the shipped args files) "
                                      "or Adagrad" % a.optimizer)
        if a.loss == 'margin-based' and a.neg_triple_num != 1:
            raise NotImplementedError("AttrE: the margin-based loss pairs one negative with a positive (losses.py:26): "
                                      "neg_triple_num = %d" % a.neg_triple_num)
        if a.loss not in ('margin-based', 'logistic', 'limited'):
            raise NotImplementedError("AttrE: loss=%s (get_loss_func knows margin-based, logistic and limited)" % a.loss)
        if a.neg_sampling != 'uniform':
            raise NotImplementedError("AttrE: neg_sampling=%s -- the reference samples the attribute triples' negatives without "
                                      "neighbours (attre.py:201) and truncated sampling is not built here" % a.neg_sampling)
        if not 1 <= a.literal_len <= ops.ATTRE_MAX_LITERAL_LEN:
            raise NotImplementedError("AttrE: literal_len %d outside 1..%d" % (a.literal_len, ops.ATTRE_MAX_LITERAL_LEN))

    def _define_variables(self):
        """attre.py:125-138: five tables"""
        a = self.args
        super()._define_variables()
        self.ent_embeds_ce = init_embeddings([self.kgs.entities_num, a.dim], 'ent_embeds_ce', a.init, a.ent_l2_norm)
        self.attr_embeds = init_embeddings([self.kgs.attributes_num, a.dim], 'attr_embeds', a.init, a.attr_l2_norm)
        self.char_embeds = init_embeddings([self.char_list_size, a.dim], 'char_embeds', a.init, a.char_l2_norm)

    def _define_embed_graph(self):
        """attre.py:140-191: the relation-triple step is BasicModel's; the character step and the joint step have an optimiser
        instance of their own each (their own Adagrad accumulators)."""
        a = self.args
        super()._define_embed_graph()
        dev = self.ent_embeds.var.device
        self.triple_loss_ce = self.triple_loss
        self.triple_optimizer_ce = ops.make_step_cfg(
            loss=a.loss, loss_norm=a.loss_norm, margin=getattr(a, 'margin', 0.0), pos_margin=getattr(a, 'pos_margin', 0.0),
            neg_margin=getattr(a, 'neg_margin', 0.0), balance=1.0,          # get_loss_func passes no balance: limited_loss's default
            ent_l2_norm=self.ent_embeds_ce.is_l2_norm, rel_l2_norm=self.attr_embeds.is_l2_norm, optimizer=a.optimizer,
            lr=a.learning_rate, neg_group_k=a.neg_triple_num)
        self.joint_loss = "sum_e (1 - ent_embeds[e] . ent_embeds_ce[e])"
        adagrad = a.optimizer == 'Adagrad'       # tf.train.AdagradOptimizer: initial_accumulator_value = 0.1
        acc = lambda t: torch.full_like(t.var, 0.1) if adagrad else None          # noqa: E731
        self._ce_acc = (acc(self.ent_embeds_ce), acc(self.attr_embeds), acc(self.char_embeds))
        self._joint_acc = (acc(self.ent_embeds), acc(self.ent_embeds_ce))
        n1, n2 = len(self.attribute_triples_list1), len(self.attribute_triples_list2)
        slot, self._attr_b1, self._attr_steps = attr_batch_layout(n1, n2, a.batch_size)
        self._attr_n = (n1, n2)
        self._attr_slot = torch.from_numpy(slot).to(dev)
        self._attr_all = ops.to_ids(np.asarray(self.attribute_triples_list1 + self.attribute_triples_list2, np.int32).reshape(-1, 3), dev)
        self._attr_dall = torch.empty((len(slot), 3), dtype=torch.int32, device=dev)
        self._attr_negs = torch.empty(len(slot) * a.neg_triple_num, dtype=torch.int32, device=dev)
        self._value_chars = ops.to_ids(self.value_id_char_ids, dev)
        n_total = self.kgs.entities_num
        self._ent_lists = []
        for kg in (self.kgs.kg1, self.kgs.kg2):
            ent_pos = np.full(n_total, -1, np.int32)
            ent_pos[np.asarray(kg.entities_list, np.int64)] = np.arange(len(kg.entities_list), dtype=np.int32)
            self._ent_lists.append((ops.to_ids(np.asarray(kg.entities_list, np.int32), dev), ops.to_ids(ent_pos, dev)))
        self._ce_ws = ops.step_workspace(self.kgs.entities_num, self.kgs.attributes_num, self.ent_embeds_ce.ld, dev)
        self._char_ws = ops.attre_char_workspace(self.char_list_size, self.char_embeds.ld, a.batch_size, dev)
        self._ce_err = torch.zeros(1, dtype=torch.int32, device=dev)
        self._ce_loss = torch.zeros(1, dtype=torch.float64, device=dev)
        self._ce_epochs = 0
        self._ce_step = 0
        # the joint step's entity list is both KGs' lists: under the sharing alignment a training pair is ONE id in both, so its
        # row is named twice (its term and its gradient count twice, as TF sums the rows of a gather)
        entities = np.asarray(self.kgs.kg1.entities_list + self.kgs.kg2.entities_list, np.int64)
        self._joint_count = ops.to_ids(np.bincount(entities, minlength=self.kgs.entities_num).astype(np.int32), dev)
        self._joint_steps = int(math.ceil(len(entities) / a.batch_size))
        self._joint_loss = torch.zeros(self._joint_steps, dtype=torch.float64, device=dev)

    def launch_triple_training_1epo_ce(self, epoch, triple_steps, steps_tasks, batch_queue):
        """attre.py:193-219.  `steps_tasks` / `batch_queue` belonged to the host producers and are ignored."""
        start = time.time()
        a = self.args
        n1, n2 = self._attr_n
        self._ce_epochs += 1
        self._layout_ws = ops.epoch_layout(self._attr_all, n1, n2, self._attr_slot, self._seed + 2, self._ce_epochs, self._attr_dall,
                                           getattr(self, "_layout_ws", None))
        b, k = a.batch_size, a.neg_triple_num
        (list1, pos1), (list2, pos2) = self._ent_lists
        for s in range(triple_steps):
            pos = self._attr_dall[s * b:(s + 1) * b]
            neg = self._attr_negs[s * b * k:(s + 1) * b * k]
            ops.attre_sample_heads(pos, self._attr_b1, k, list1, pos1, list2, pos2, self._seed + 3, self._ce_step, out=neg)
            self._ce_step += 1
            ops.attre_char_step(self.ent_embeds_ce.var, self._ce_acc[0], self.attr_embeds.var, self._ce_acc[1], self.char_embeds.var,
                                self._ce_acc[2], a.dim, self._value_chars, pos, neg, self.char_embeds.is_l2_norm,
                                self.triple_optimizer_ce, self._ce_ws, self._char_ws, self._ce_err, self._ce_loss,
                                char_path=self.char_path)
        ops.attre_check(self._ce_err)
        epoch_loss = float(self._ce_loss.item()) / max(triple_steps * b, 1)
        self._ce_loss.zero_()
        print('epoch {}, CE, avg. triple loss: {:.4f}, cost time: {:.4f}s'.format(epoch, epoch_loss, time.time() - start))
        return epoch_loss

    def launch_joint_training_1epo(self, epoch, entities):
        """attre.py:221-233: ceil(|entities| / batch_size) steps, each over all entities"""
        start = time.time()
        a = self.args
        steps = int(math.ceil(len(entities) / a.batch_size))
        assert steps == self._joint_steps
        ops.attre_joint_epoch(self.ent_embeds.var, self._joint_acc[0], self.ent_embeds_ce.var, self._joint_acc[1], a.dim,
                              self.ent_embeds.is_l2_norm, a.optimizer, a.learning_rate, steps, self._joint_loss, self._joint_count)
        epoch_loss = float(self._joint_loss.sum().item()) / max(steps * len(entities), 1)
        self._joint_loss.zero_()
        print('epoch {}, joint learning loss: {:.4f}, time: {:.4f}s'.format(epoch, epoch_loss, time.time() - start))
        return epoch_loss

    def run(self):
        """attre.py:235-257"""
        t = time.time()
        relation_triples_num = len(self.kgs.kg1.relation_triples_list) + len(self.kgs.kg2.relation_triples_list)
        attribute_triples_num = len(self.attribute_triples_list1) + len(self.attribute_triples_list2)
        relation_triple_steps = int(math.ceil(relation_triples_num / self.args.batch_size))
        attribute_triple_steps = int(math.ceil(attribute_triples_num / self.args.batch_size))
        relation_step_tasks = task_divide(list(range(relation_triple_steps)), self.args.batch_threads_num)
        attribute_step_tasks = task_divide(list(range(attribute_triple_steps)), self.args.batch_threads_num)
        entity_list = list(self.kgs.kg1.entities_list + self.kgs.kg2.entities_list)
        for i in range(1, self.args.max_epoch + 1):
            self.launch_triple_training_1epo(i, relation_triple_steps, relation_step_tasks, None, None, None)
            self.launch_triple_training_1epo_ce(i, attribute_triple_steps, attribute_step_tasks, None)
            self.launch_joint_training_1epo(i, entity_list)
            if i >= self.args.start_valid and i % self.args.eval_freq == 0:
                flag = self.valid(self.args.stop_metric)
                self.flag1, self.flag2, self.early_stop = early_stop(self.flag1, self.flag2, flag)
                if self.early_stop or i == self.args.max_epoch:
                    break
        if self._epochs is not None:
            self._epochs.check()
        print("Training ends. Total time = {:.3f} s.".format(time.time() - t))
