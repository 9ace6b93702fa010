"""Attr2Vec (mirror of openea/approaches/attr2vec.py:19-194): JAPE's attribute embedding, a skip-gram over the attributes that
co-occur on an entity (or on the two ends of a training link) under tf.nn.nce_loss and Adagrad.

The host functions keep the reference's set and dict iteration order: itertools.combinations over a python set decides which of
(a, c) / (c, a) is the input and which the label.  The training step is oea_attr2vec_step / oea_attr2vec_epoch
(csrc/attr2vec_step.hip); random.sample of the reference (attr2vec.py:150) is the keyed permutation of oea_sample_distinct and
the candidate sampler of nce_loss the log-uniform sampler of ProjE, both pure functions of (seed, step).

`run` calls generate_training_data(self.kgs, threshold=0.9) with the reference's literal 0.9 (attr2vec.py:185), not
args.top_attr_threshold."""
import itertools
import time
from collections import Counter

import numpy as np
import torch

from .. import ops
from ..modules.base.initializers import xavier_init
from ..modules.finding import evaluation
from ..modules.load import read
from ..modules.utils.util import generate_out_folder, merge_dic


def get_kg_popular_attributes(kg, threshold):
    """attr2vec.py:19-28 -> the int(threshold * #attributes) most frequent attributes of one KG as a set.  Attributes of equal
    frequency rank in the order of their first triple in kg.attribute_triples_list, as the reference's stable descending sort of
    a dict filled in that order ranks them."""
    frequency = Counter(triple[1] for triple in kg.attribute_triples_list)       # a dict: first-seen order
    print("total attributes:", len(frequency))
    ranked = sorted(frequency, key=lambda attribute: -frequency[attribute])      # stable: ties stay in first-seen order
    popular = set(ranked[:int(len(frequency) * threshold)])
    print("selected attributes", len(popular))
    return popular


def get_kgs_popular_attributes(kgs, threshold):
    """attr2vec.py:31-36 -> (KG1's popular attributes, KG2's, their union)"""
    popular = [get_kg_popular_attributes(kg, threshold) for kg in (kgs.kg1, kgs.kg2)]
    union = popular[0] | popular[1]
    print("total selected attributes", len(union))
    return popular[0], popular[1], union


def generate_training_data(kgs, threshold=1.0):
    """attr2vec.py:39-55 -> the list of (input, label) attribute pairs: for every entity that has attributes -- KG1's entities
    first, each KG's in the order of its entity_attributes_dict --, every 2-combination of its selected attributes, where an
    entity of a training link also counts its counterpart's.  Which attribute of a pair comes first is the order in which python
    walks the set ((own | counterpart's) & selected, built in exactly that way), so the set expressions stay as the reference's."""
    selected = get_kgs_popular_attributes(kgs, threshold)[2]
    held = merge_dic(kgs.kg1.entity_attributes_dict, kgs.kg2.entity_attributes_dict)
    print("entity attribute dict", len(held))
    counterpart = dict(zip(kgs.train_entities1, kgs.train_entities2))
    counterpart.update(zip(kgs.train_entities2, kgs.train_entities1))
    pairs = []
    for entity, own in held.items():
        pool = own | held.get(counterpart[entity], set()) if entity in counterpart else own
        pool = pool & selected
        pairs.extend(pair for pair in itertools.combinations(pool, 2) if pair[0] != pair[1])
    print("training data of attribute correlations", len(pairs))
    return pairs


def entity_attribute_csr(kgs, selected_attributes):
    """the mean over an entity's selected attributes as a CSR [entities_num, attributes_num] with the values 1 / count (host int32 /
    fp32 arrays); an entity without selected attributes has an empty row"""
    entity_attributes_dict = merge_dic(kgs.kg1.entity_attributes_dict, kgs.kg2.entity_attributes_dict)
    rowptr = np.zeros(kgs.entities_num + 1, np.int32)
    cols, vals = [], []
    for i in range(kgs.entities_num):
        attributes = list(entity_attributes_dict.get(i, set()) & selected_attributes)
        cols.extend(attributes)
        if attributes:
            vals.extend([1.0 / len(attributes)] * len(attributes))
        rowptr[i + 1] = len(cols)
    return rowptr, np.asarray(cols, np.int32), np.asarray(vals, np.float32)


def get_ent_embeds_from_attributes_device(kgs, attr_embeds, dim, selected_attributes):
    """attr2vec.py:58-76 on the device: attr_embeds device [A, ld] (the table as .eval() shows it) -> device [entities_num, ld],
    the mean row per entity (oea_spmm_csr with 1 / count) under sklearn's normalize (a zero row stays zero)"""
    dev = attr_embeds.device
    rowptr, cols, vals = entity_attribute_csr(kgs, selected_attributes)
    mat = ops.spmm_csr(ops.to_ids(rowptr, dev), ops.to_ids(cols, dev), ops.to_vec(vals, dev), attr_embeds, dim)
    return ops.normalize_rows_(mat, dim, sklearn=True)


def get_ent_embeds_from_attributes(kgs, attr_embeds, selected_attributes):
    """attr2vec.py:58-76: host [A, d] -> host [entities_num, d]"""
    print("get entity embeddings from attributes")
    start = time.time()
    attr_embeds = np.asarray(attr_embeds, np.float32)
    mat = get_ent_embeds_from_attributes_device(kgs, ops.to_table(attr_embeds), attr_embeds.shape[1], selected_attributes)
    print('cost time: {:.4f}s'.format(time.time() - start))
    return mat[:, :attr_embeds.shape[1]].cpu().numpy()


class Attr2Vec:
    def set_kgs(self, kgs):
        self.kgs = kgs
        _, _, self.selected_attributes = get_kgs_popular_attributes(kgs, self.args.top_attr_threshold)
        self.num_sampled_negs = len(self.selected_attributes) // 5

    def set_args(self, args):
        self.args = args
        self.out_folder = generate_out_folder(self.args.output, self.args.training_data, self.args.dataset_division,
                                              self.__class__.__name__)

    def init(self):
        self._check_device_path()
        self._define_variables()
        self._define_embed_graph()

    def __init__(self):
        self.num_sampled_negs = -1
        self.kgs = None
        self.args = None
        self.out_folder = None
        self.flag1, self.flag2 = -1, -1
        self.early_stop = False
        self.session = None
        self.selected_attributes = None
        self.opt = 'Adagrad'
        self._seed = 0

    def _check_device_path(self):
        """the limits of the step, raised before any table is made"""
        if self.args.dim > ops.JAPE_MAX_DIM:
            raise NotImplementedError("Attr2Vec: dim %d > %d (the step holds a row in two columns per lane of one wave)"
                                      % (self.args.dim, ops.JAPE_MAX_DIM))
        if self.kgs.attributes_num > ops.LOG_UNIFORM_STEPS_MAX_CLASSES:
            raise NotImplementedError("Attr2Vec: %d attributes > %d (the per-epoch candidate sampler keeps its table in LDS)"
                                      % (self.kgs.attributes_num, ops.LOG_UNIFORM_STEPS_MAX_CLASSES))
        if not 1 <= self.num_sampled_negs <= self.kgs.attributes_num:
            raise ValueError("Attr2Vec: %d sampled negatives of %d attributes (|selected| // 5 must be at least 1)"
                             % (self.num_sampled_negs, self.kgs.attributes_num))

    def _define_variables(self):
        """attr2vec.py:106-111"""
        n, d = self.kgs.attributes_num, self.args.dim
        self.embeds = xavier_init([n, d], 'attr_embed', True)
        self.nce_weights = xavier_init([n, d], 'nce_weights', True)
        self.nce_biases = torch.zeros(n, dtype=torch.float32, device=self.embeds.var.device)

    def _define_embed_graph(self):
        """attr2vec.py:113-124: mean nce_loss under Adagrad (initial accumulator 0.1)"""
        dev = self.embeds.var.device
        self.loss = "mean_b softplus(-true_b) + sum_j softplus(samp_bj)"
        self._vars = [self.embeds.var, self.nce_weights.var, self.nce_biases]
        self._accs = [torch.full_like(v, 0.1) for v in self._vars]
        self.optimizer = self.opt
        self._thresholds = ops.log_uniform_thresholds(self.kgs.attributes_num, dev)
        self._ws = ops.attr2vec_workspace(self.kgs.attributes_num, self.embeds.ld, self.num_sampled_negs, dev)
        self._loss = torch.zeros(1, dtype=torch.float64, device=dev)
        self._buffers = None
        self._step = 0

    def eval_attribute_embeddings(self):
        return self.embeds.eval()

    def _ent_mat(self):
        ids = torch.arange(self.embeds.rows, dtype=torch.int32, device=self.embeds.var.device)
        return get_ent_embeds_from_attributes_device(self.kgs, self.embeds.lookup(ids), self.args.dim, self.selected_attributes)

    def _rows(self, mat, ids):
        return mat[ops.to_ids(np.asarray(ids, np.int32), mat.device).long()].contiguous()

    def eval_kg1_ent_embeddings(self):
        return self._rows(self._ent_mat(), self.kgs.kg1.entities_list)[:, :self.args.dim].cpu().numpy()

    def eval_kg2_ent_embeddings(self):
        return self._rows(self._ent_mat(), self.kgs.kg2.entities_list)[:, :self.args.dim].cpu().numpy()

    def _ref_embeds(self):
        mat = self._ent_mat()
        return (self._rows(mat, self.kgs.valid_entities1 + self.kgs.test_entities1),
                self._rows(mat, self.kgs.valid_entities2 + self.kgs.test_entities2))

    def eval_sim_mat(self):
        """attr2vec.py:139-143: the dense [n_ref, n_ref] numpy matrix (API parity; JAPE takes eval_sim_csr)"""
        embeds1, embeds2 = self._ref_embeds()
        return ops.sim_matrix(embeds1, embeds2, self.args.dim, 'inner').cpu().numpy()

    def eval_sim_csr(self, threshold, block_rows=4096):
        """the entries >= threshold of that matrix as a device CSR (indptr int64, col int32, val fp32), one block of rows dense at
        a time"""
        embeds1, embeds2 = self._ref_embeds()
        return ops.sim_csr(embeds1, embeds2, self.args.dim, threshold, block_rows=block_rows)

    def launch_training_1epo(self, epoch, steps, training_data_list):
        """attr2vec.py:145-161: `steps` batches of batch_size sampled pairs; the printed loss is the sum of the batch means.
        training_data_list: the host list, or the device int32 [n, 2] tensor `run` made of it."""
        start = time.time()
        if steps == 0:                    # fewer pairs than one batch: the reference's loop body never runs and it prints 0
            print('epoch {}, attribute loss: {:.4f}, cost time: {:.4f}s'.format(epoch, 0.0, time.time() - start))
            return 0.0
        if not hasattr(training_data_list, "is_cuda"):
            training_data_list = ops.to_ids(np.asarray(training_data_list, np.int32).reshape(-1, 2), self.embeds.var.device)
        if self._buffers is not None and self._buffers[0].shape[0] != steps:
            self._buffers = None
        self._buffers = ops.attr2vec_epoch(self._vars, self._accs, self.args.dim, training_data_list, self.args.batch_size, steps,
                                           self._seed, self._step, self._thresholds, self.num_sampled_negs,
                                           self.args.learning_rate, self._ws, self._loss, self._buffers)
        self._step += steps
        epoch_loss = float(self._loss.item())
        self._loss.zero_()
        failed = int(self._buffers[3].count_nonzero())
        if failed:                        # those steps changed nothing (their kernels return at once on the status word)
            raise ops.OpenEAHipError("Attr2Vec: in %d of %d steps the candidate sampler did not reach %d distinct attributes of %d "
                                     "in 64 x as many draws" % (failed, steps, self.num_sampled_negs, self.kgs.attributes_num))
        print('epoch {}, attribute loss: {:.4f}, cost time: {:.4f}s'.format(epoch, epoch_loss, time.time() - start))
        return epoch_loss

    def valid(self):
        mat = self._ent_mat()
        embeds1, embeds2 = self._rows(mat, self.kgs.valid_entities1), self._rows(mat, self.kgs.valid_entities2)
        embeds1.oea_dim = embeds2.oea_dim = self.args.dim
        hits1_12, mrr_12 = evaluation.valid(embeds1, embeds2, None, self.args.top_k, self.args.test_threads_num,
                                            metric=self.args.eval_metric)
        if self.args.stop_metric == 'hits1':
            return hits1_12
        return mrr_12

    def test(self, save=True):
        mat = self._ent_mat()
        embeds1, embeds2 = self._rows(mat, self.kgs.test_entities1), self._rows(mat, self.kgs.test_entities2)
        embeds1.oea_dim = embeds2.oea_dim = self.args.dim
        rest_12, _, _ = evaluation.test(embeds1, embeds2, None, self.args.top_k, self.args.test_threads_num,
                                        metric=self.args.eval_metric, csls_k=self.args.csls)
        if save:
            ent_ids_rest_12 = [(self.kgs.test_entities1[i], self.kgs.test_entities2[j]) for i, j in rest_12]
            read.save_results(self.out_folder, ent_ids_rest_12)

    def run(self):
        training_data_list = generate_training_data(self.kgs, threshold=0.9)        # the reference's literal (attr2vec.py:185)
        steps = len(training_data_list) // self.args.batch_size
        pairs = ops.to_ids(np.asarray(training_data_list, np.int32).reshape(-1, 2), self.embeds.var.device) if steps else None
        for i in range(1, self.args.attr_max_epoch + 1):
            self.launch_training_1epo(i, steps, pairs)

    def save(self):
        read.save_embeddings(self.out_folder, self.kgs, None, None, self.embeds.eval())
