"""MultiKE (mirror of openea/approaches/multi_ke.py:318-929): three views of an entity -- its name (a constant literal vector), its
relation triples (a logistic translational model) and its attribute triples (a small CNN over (attribute, value) pairs) -- tied
to one shared table by cross-view terms, plus cross-KG steps on the seed-swapped triples and on triples whose predicate was swapped
for its soft-aligned partner (approaches/predicate_alignmnet.py).

Where the work runs: the relation view's logistic loss is the step engine's (PHASE_GRAD), its cross-view terms, the common-space
pull and the weighted softplus positive are oea_multike_rows, every `conv()` graph is oea_multike_cnn_step (csrc/multike_step.hip:
four independent parameter sets, as tf.layers makes fresh variables on each of the reference's four calls); all of them leave
gradients w.r.t. the normalised rows in the engine's scratch and the engine's apply phase runs SGD through the normalisation.

Deliberate differences:
  * ORDER.  Where the reference orders by `list(set(...))` (the literal list, the value ids, the weighted triple lists) the order
    here is sorted; with PYTHONHASHSEED unset the reference's own order changes from run to run.
  * SHUFFLE.  As AttrE: every epoch draws a fresh keyed permutation of the attribute lists as loaded (oea_epoch_layout), the
    relation lists go through the engine's epoch batches; random.sample is oea_sample_distinct.
  * LITERALS.  LiteralEncoder needs the word-vector file and gensim.  `literal_encoder` is a callable literal_list -> float [n, dim];
    when it is None, args.literal_vectors_path names an .npz with `literals` and `vectors`.  Neither: NotImplementedError.
  * WEIGHTS.  A triple's weight is a function of its predicate id (predicate_alignmnet.py), so a float vector per predicate
    table travels to the device, not a weight per triple.
  * 2 x positive_loss of the cross-KG entity step runs as the engine's 'positive' loss under twice the learning rate (SGD: the same
    update); the reported loss is doubled.
Not built (NotImplementedError before any table is made): _define_space_mapping_graph and its step (the reference never runs
them, multi_ke.py:923-927), optimisers other than SGD, neg_sampling='truncated', dim > 128, more than one torch.distributed rank."""
import math
import time
import types

import numpy as np
import torch

from .. import ops
from ..models.basic_model import BasicModel
from ..models.trainer import EmbeddingTable, RelationTripleEpochs
from ..modules.base import initializers
from ..modules.base.initializers import init_embeddings
from ..modules.finding.evaluation import early_stop
from ..modules.load.read import generate_sup_attribute_triples
from .predicate_alignmnet import PredicateAlignModel


def is_number(s):
    """multi_ke.py:239-251"""
    try:
        float(s)
        return True
    except ValueError:
        pass
    try:
        import unicodedata
        unicodedata.numeric(s)
        return True
    except (TypeError, ValueError):
        pass
    return False


def clear_attribute_triples(attribute_triples):
    """multi_ke.py:193-236: attributes with fewer than ten triples go, the values lose their quotes, datatype and language tags and
    punctuation, values that hold 'http' go -> (triples, the numeric literals, the other literals).  Step 1 builds a set; it is
    walked in sorted order here."""
    attr_num = {}
    for (_, a, _) in attribute_triples:
        attr_num[a] = attr_num.get(a, 0) + 1
    kept = set(t for t in attribute_triples if attr_num[t[1]] >= 10)
    attribute_triples_new = []
    literals_number, literals_string = [], []
    for (e, a, v) in sorted(kept):
        v = v.strip('"')
        if '"^^' in v:
            v = v[:v.index('"^^')]
        if v.endswith('"@en'):
            v = v[:v.index('"@en')]
        if v.endswith('"@eng'):
            v = v[:v.index('"@eng')]
        if is_number(v):
            literals_number.append(v)
        else:
            literals_string.append(v)
        v = v.replace('.', '').replace('(', '').replace(')', '').replace(',', '').replace('"', '')
        v = v.replace('_', ' ').replace('-', ' ').replace('/', ' ')
        if 'http' in v:
            continue
        attribute_triples_new.append((e, a, v))
    return attribute_triples_new, literals_number, literals_string


def _normalize_rows(mat):
    """sklearn.preprocessing.normalize: a zero row stays zero"""
    norm = np.linalg.norm(mat, axis=1, keepdims=True)
    return mat / np.where(norm == 0, 1.0, norm)


def attribute_batch_layout(n1, n2, batch_size, steps):
    """generate_attribute_triple_batch (multi_ke.py:280-291) with bat.generate_pos_triples' slice rule (batch.py:48-53) as a gather map
    over cat(list1, list2) -> (slot int64, offsets int64 [steps + 1]): step s reads slot[offsets[s]:offsets[s + 1]] = list1[s b1 :
    s b1 + b1] then list2[s b2 : s b2 + b2], each cut at its list's end (a late step may be short or empty)."""
    b1 = int(n1 / (n1 + n2) * batch_size) if n1 + n2 else 0
    b2 = batch_size - b1
    slot, offsets = [], [0]
    for s in range(steps):
        slot.append(np.arange(min(s * b1, n1), min(s * b1 + b1, n1), dtype=np.int64))
        slot.append(np.arange(min(s * b2, n2), min(s * b2 + b2, n2), dtype=np.int64) + n1)
        offsets.append(offsets[-1] + len(slot[-2]) + len(slot[-1]))
    return (np.concatenate(slot) if slot else np.zeros(0, np.int64)), np.asarray(offsets, np.int64)


def valid_temp(model, embed_choice='avg', w=(1, 1, 1)):
    """multi_ke.py:129-151 through ops.rank_eval on the normalised rows -> mrr"""
    if embed_choice == 'nv':
        table = model.name_embeds
    elif embed_choice == 'rv':
        table = model.rv_ent_embeds
    elif embed_choice == 'av':
        table = model.av_ent_embeds
    elif embed_choice == 'final':
        table = model.ent_embeds
    else:
        raise NotImplementedError("valid_temp: embed_choice=%r (the reference runs 'nv', 'rv' and 'av')" % (embed_choice,))
    print(embed_choice, 'valid results:')
    dev, dim, kgs = table.var.device, model.args.dim, model.kgs
    e1 = ops.gather_rows(table.var, dim, ops.to_ids(np.asarray(kgs.valid_entities1, np.int32), dev), normalize=True)
    e2 = ops.gather_rows(table.var, dim, ops.to_ids(np.asarray(kgs.valid_entities2 + kgs.test_entities2, np.int32), dev), normalize=True)
    if e1.shape[0] == 0:
        return 0.0
    rank, _ = ops.rank_eval(e1, e2, dim, metric='inner')
    hits, rank_sum, rr_sum = ops.rank_metrics(rank, model.args.top_k)
    n = e1.shape[0]
    print("quick results: hits@{} = {}%, mr = {:.3f}, mrr = {:.6f}".format(model.args.top_k, [round(100.0 * h / n, 3) for h in hits],
                                                                            rank_sum / n, rr_sum / n))
    return rr_sum / n


class MultiKE(BasicModel):

    def __init__(self):
        super().__init__()
        self.literal_encoder = None
        self.history = {}

    # ---- host side -------------------------------------------------------------------------------------------------------------
    def init(self):
        self._check_device_path()
        self.entities = self.kgs.kg1.entities_set | self.kgs.kg2.entities_set
        self.entity_local_name_dict = self._get_local_name_by_name_triple()
        print('len(self.entity_local_name_dict):', len(self.entity_local_name_dict))
        self._generate_literal_vectors()
        self._generate_name_vectors_mat()
        self._generate_attribute_value_vectors()
        self.predicate_align_model = PredicateAlignModel(self.kgs, self.args)
        self._define_variables()
        self._define_relation_view_graph()
        self._define_attribute_view_graph()
        self._define_cross_kg_entity_reference_relation_view_graph()
        self._define_cross_kg_entity_reference_attribute_view_graph()
        self._define_cross_kg_relation_reference_graph()
        self._define_cross_kg_attribute_reference_graph()
        self._define_common_space_learning_graph()

    def _check_device_path(self):
        """what is not built, raised before any table is made"""
        a = self.args
        if self._dist_group() is not None:
            raise NotImplementedError("MultiKE runs on one GPU (launch it without torch.distributed, or with one rank)")
        if a.dim > ops.MULTIKE_MAX_DIM:
            raise NotImplementedError("MultiKE: dim %d > %d (the steps hold a row in two columns per lane of one wave)"
                                      % (a.dim, ops.MULTIKE_MAX_DIM))
        if a.optimizer != 'SGD':
            raise NotImplementedError("MultiKE: optimizer=%s -- the CNN's parameters train with SGD (both shipped args files)" % a.optimizer)
        if a.neg_sampling == 'truncated':
            raise NotImplementedError("MultiKE: neg_sampling='truncated' is not built (the shipped args files sample uniformly)")
        if self.literal_encoder is None and not getattr(a, 'literal_vectors_path', None):
            raise NotImplementedError("MultiKE: LiteralEncoder (the word-vector file and gensim) is not built: set model.literal_encoder "
                                      "to a callable literal_list -> float [n, dim], or args.literal_vectors_path to an .npz with "
                                      "`literals` and `vectors`")

    def _define_space_mapping_graph(self):
        raise NotImplementedError("MultiKE: the space-mapping graph (multi_ke.py:640-658) is not built: the reference never runs its step "
                                  "(multi_ke.py:923-927)")

    def train_shared_space_mapping_1epo(self, epoch, entities):
        self._define_space_mapping_graph()

    def _get_local_name_by_name_triple(self, name_attribute_list=None):
        """multi_ke.py:344-393: an entity's name is the value of a name attribute, else the last segment of its URI"""
        if name_attribute_list is None:
            if 'D_Y' in self.args.training_data:
                name_attribute_list = {'skos:prefLabel', 'http://dbpedia.org/ontology/birthName'}
            elif 'D_W' in self.args.training_data:
                name_attribute_list = {'http://www.wikidata.org/entity/P373', 'http://www.wikidata.org/entity/P1476'}
            else:
                name_attribute_list = {}
        kg1, kg2 = self.kgs.kg1, self.kgs.kg2
        triples = []
        for h, a, v in sorted(set(kg1.local_attribute_triples_list) | set(kg2.local_attribute_triples_list)):
            v = v.strip('"')
            if v.endswith('"@eng'):
                v = v.rstrip('"@eng')
            triples.append((h, a, v))
        id_ent_dict = {}
        for e, e_id in kg1.entities_id_dict.items():
            id_ent_dict[e_id] = e
        for e, e_id in kg2.entities_id_dict.items():
            id_ent_dict[e_id] = e
        name_ids = set()
        for ids in (kg1.attributes_id_dict, kg2.attributes_id_dict):
            for a, a_id in ids.items():
                if a in name_attribute_list:
                    name_ids.add(a_id)
        local_name_dict = {}
        for (e, a, v) in triples:
            if a in name_ids:
                local_name_dict[id_ent_dict[e]] = v
        for e in sorted(kg1.entities_set | kg2.entities_set):
            if id_ent_dict[e] not in local_name_dict:
                local_name_dict[id_ent_dict[e]] = id_ent_dict[e].split('/')[-1].replace('_', ' ')
        return local_name_dict

    def _generate_literal_vectors(self):
        """multi_ke.py:395-410 with the encoder replaced (module docstring); the literal list is sorted"""
        cleaned1, _, _ = clear_attribute_triples(self.kgs.kg1.local_attribute_triples_list)
        cleaned2, _, _ = clear_attribute_triples(self.kgs.kg2.local_attribute_triples_list)
        self._cleaned = (cleaned1, cleaned2)
        value_list = [v for (_, _, v) in cleaned1 + cleaned2]
        local_name_list = list(self.entity_local_name_dict.values())
        self.literal_list = sorted(set(value_list + local_name_list))
        print('literal num:', len(local_name_list), len(value_list), len(self.literal_list))
        if self.literal_encoder is not None:
            mat = np.asarray(self.literal_encoder(self.literal_list), np.float32)
        else:
            z = np.load(self.args.literal_vectors_path, allow_pickle=False)
            index = {l: i for i, l in enumerate(z['literals'].tolist())}
            missing = [l for l in self.literal_list if l not in index]
            if missing:
                raise ValueError("MultiKE: %d of %d literals have no vector in %s" % (len(missing), len(self.literal_list),
                                                                                      self.args.literal_vectors_path))
            mat = np.asarray(z['vectors'], np.float32)[[index[l] for l in self.literal_list]]
        if mat.shape != (len(self.literal_list), self.args.dim):
            raise ValueError("MultiKE: literal vectors of shape %r for %d literals at dim %d" % (mat.shape, len(self.literal_list),
                                                                                               self.args.dim))
        self.literal_vectors_mat = mat
        self.literal_id_dic = {l: i for i, l in enumerate(self.literal_list)}

    def _generate_name_vectors_mat(self):
        """multi_ke.py:412-433"""
        entity_id_uris_dic = dict(zip(self.kgs.kg1.entities_id_dict.values(), self.kgs.kg1.entities_id_dict.keys()))
        entity_id_uris_dic.update(dict(zip(self.kgs.kg2.entities_id_dict.values(), self.kgs.kg2.entities_id_dict.keys())))
        num = len(self.entities)
        assert len(entity_id_uris_dic) == num
        name_ordered_list = [self.literal_id_dic[self.entity_local_name_dict[entity_id_uris_dic[i]]] for i in range(num)]
        name_mat = self.literal_vectors_mat[name_ordered_list]
        if self.args.literal_normalize:
            name_mat = _normalize_rows(name_mat)
        self.local_name_vectors = name_mat

    def _generate_attribute_value_vectors(self):
        """multi_ke.py:435-475; the value ids follow the sorted values"""
        self.literal_set = set(self.literal_list)
        cleaned1, cleaned2 = self._cleaned
        triples1 = set((h, a, v) for h, a, v in cleaned1 if v in self.literal_set)
        triples2 = set((h, a, v) for h, a, v in cleaned2 if v in self.literal_set)
        print("selected attribute triples", len(triples1), len(triples2))
        values_list = sorted(set(v for (_, _, v) in triples1 | triples2))
        if not values_list:
            raise ValueError("MultiKE: no attribute triple is left after clear_attribute_triples (attributes need ten triples)")
        values_id_dic = {v: i for i, v in enumerate(values_list)}
        self.kgs.kg1.set_attributes(set((h, a, values_id_dic[v]) for (h, a, v) in triples1))
        self.kgs.kg2.set_attributes(set((h, a, values_id_dic[v]) for (h, a, v) in triples2))
        sup_triples1, sup_triples2 = generate_sup_attribute_triples(self.kgs.train_links, self.kgs.kg1.av_dict, self.kgs.kg2.av_dict)
        self.kgs.kg1.add_sup_attribute_triples(sup_triples1)
        self.kgs.kg2.add_sup_attribute_triples(sup_triples2)
        value_vectors = self.literal_vectors_mat[[self.literal_id_dic[v] for v in values_list]]
        if self.args.literal_normalize:
            value_vectors = _normalize_rows(value_vectors)
        self.value_vectors = value_vectors

    # ---- variables and graphs ----------------------------------------------------------------------------------------------------
    def _cnn_variables(self, dev):
        """the eight variables of one `conv()` call as tf.layers creates them: gamma 1, beta 0, glorot-uniform kernels and dense
        weights, zero biases (ops.MULTIKE_VARS)"""
        d, ld, rng = self.args.dim, ops.pad4(self.args.dim), initializers._rng

        def glorot(shape, fan_in, fan_out):
            lim = math.sqrt(6.0 / (fan_in + fan_out))
            return rng.uniform(-lim, lim, shape).astype(np.float32)
        host = [np.ones(d, np.float32), np.zeros(d, np.float32), glorot((2, 4, 1, 2), 8, 16), np.zeros(2, np.float32),
                glorot((2, 4, 2, 2), 16, 16), np.zeros(2, np.float32), glorot((4 * d, d), 4 * d, d), np.zeros(d, np.float32)]
        return [ops.to_table(h, ld=ld, dev=dev) if i == 6 else ops.to_vec(h.reshape(-1), dev) for i, h in enumerate(host)]

    def _define_variables(self):
        """multi_ke.py:477-498 without the three space mappings"""
        a, E = self.args, self.kgs.entities_num
        self.literal_embeds = EmbeddingTable(self.value_vectors, False, 'literal_embeds')
        self.name_embeds = EmbeddingTable(self.local_name_vectors, False, 'name_embeds')
        self.rv_ent_embeds = init_embeddings([E, a.dim], 'rv_ent_embeds', 'xavier', True)
        self.rel_embeds = init_embeddings([self.kgs.relations_num, a.dim], 'rel_embeds', 'xavier', True)
        self.av_ent_embeds = init_embeddings([E, a.dim], 'av_ent_embeds', 'xavier', True)
        self.attr_embeds = init_embeddings([self.kgs.attributes_num, a.dim], 'attr_embeds', 'xavier', False)      # "False important!"
        self.ent_embeds = init_embeddings([E, a.dim], 'ent_embeds', 'xavier', True)
        dev, ld = self.ent_embeds.var.device, self.ent_embeds.ld
        self._dev = dev
        self._ws_rv = ops.step_workspace(E, self.kgs.relations_num, ld, dev)
        self._ws_av = ops.step_workspace(E, self.kgs.attributes_num, ld, dev)
        self._ws_f = ops.step_workspace(E, 1, ld, dev)
        self._dummy_rel = torch.zeros((1, ld), dtype=torch.float32, device=dev)
        self._empty = torch.zeros((0, 3), dtype=torch.int32, device=dev)
        self._sink = torch.zeros(1, dtype=torch.float64, device=dev)
        self._loss = torch.zeros(1, dtype=torch.float64, device=dev)
        self._draws = 0
        max_n = max(int(a.attribute_batch_size), 1)
        self._cnn_ws = ops.multike_cnn_workspace(a.dim, ld, max_n, dev)
        self._upload_weights()

    def _cfg(self, lr, rel_l2_norm, loss='positive', k=0):
        return ops.make_step_cfg(loss=loss, loss_norm='L2', ent_l2_norm=True, rel_l2_norm=rel_l2_norm, optimizer='SGD', lr=lr, neg_group_k=k)

    def _upload_weights(self):
        """the weight vectors and the predicate-swapped triple lists of the current predicate alignment"""
        pm, dev = self.predicate_align_model, self._dev
        self._attr_w = ops.to_vec(pm.attribute_weights, dev)
        self._sup_attr_w = ops.to_vec(pm.sup_attribute_weights, dev)
        self._sup_rel_w = ops.to_vec(pm.sup_relation_weights, dev)
        ids = lambda rows: ops.to_ids(np.asarray([r[:3] for r in rows], np.int32).reshape(-1, 3), dev)    # noqa: E731
        self._ckgp_rel = ids(pm.sup_relation_alignment_triples1 + pm.sup_relation_alignment_triples2)
        self._ckga_attr = ids(pm.sup_attribute_alignment_triples1 + pm.sup_attribute_alignment_triples2)

    def _define_relation_view_graph(self):
        """multi_ke.py:502-530"""
        a, kgs = self.args, self.kgs
        self.relation_loss = "logistic_loss + cross-view terms"
        self._rv_cfg = self._cfg(a.learning_rate, True, 'logistic', a.neg_triple_num)
        self._f_cfg = self._cfg(a.learning_rate, False)
        side = lambda kg: types.SimpleNamespace(relation_triples_list=kg.local_relation_triples_list,         # noqa: E731
                                                relation_triples_set=kg.local_relation_triples_set, entities_list=kg.entities_list)
        shim = types.SimpleNamespace(kg1=side(kgs.kg1), kg2=side(kgs.kg2), entities_num=kgs.entities_num)
        self._rel_epochs = RelationTripleEpochs(shim, a.batch_size, a.neg_triple_num, seed=self._seed, dev=self._dev)

    def _define_attribute_view_graph(self):
        """multi_ke.py:532-555: two nets on one batch"""
        a, pm, dev = self.args, self.predicate_align_model, self._dev
        self.attribute_loss = "sum w softplus(|av - cnn|^2) + sum softplus(|f - cnn|^2) + 0.5 |f - name|^2"
        self._av_cfg = self._cfg(a.learning_rate, False)
        A = self.kgs.attributes_num
        self._cnn_av = ops.multike_net(self._cnn_variables(dev), self.av_ent_embeds.var, self._ws_av, A, weighted=True)
        self._cnn_f = ops.multike_net(self._cnn_variables(dev), self.ent_embeds.var, self._ws_f, 1, weighted=False)
        list1 = [t[:3] for t in pm.attribute_triples_w_weights1]
        list2 = [t[:3] for t in pm.attribute_triples_w_weights2]
        self._attr_n = (len(list1), len(list2))
        self._attr_all = ops.to_ids(np.asarray(list1 + list2, np.int32).reshape(-1, 3), dev)
        self._attr_epochs = 0
        self._attr_layout = None

    def _define_cross_kg_entity_reference_relation_view_graph(self):
        """multi_ke.py:559-571"""
        kg1, kg2 = self.kgs.kg1, self.kgs.kg2
        self.ckge_relation_loss = "2 * positive_loss"
        self._ckge_rel_cfg = self._cfg(2.0 * self.args.learning_rate, True)
        sup = (kg1.sup_relation_triples_list or []) + (kg2.sup_relation_triples_list or [])
        self._ckge_rel = ops.to_ids(np.asarray(sup, np.int32).reshape(-1, 3), self._dev)

    def _define_cross_kg_entity_reference_attribute_view_graph(self):
        """multi_ke.py:573-586"""
        kg1, kg2 = self.kgs.kg1, self.kgs.kg2
        self.ckge_attribute_loss = "2 * sum softplus(|av - cnn|^2)"
        self._cnn_ckge = ops.multike_net(self._cnn_variables(self._dev), self.av_ent_embeds.var, self._ws_av, self.kgs.attributes_num,
                                         weighted=False, factor=2.0)
        sup = (kg1.sup_attribute_triples_list or []) + (kg2.sup_attribute_triples_list or [])
        self._ckge_attr = ops.to_ids(np.asarray(sup, np.int32).reshape(-1, 3), self._dev)

    def _define_cross_kg_relation_reference_graph(self):
        """multi_ke.py:588-602"""
        self.ckgp_relation_loss = "2 * positive_loss_with_weight"
        self._ckgp_cfg = self._cfg(self.args.learning_rate, True)

    def _define_cross_kg_attribute_reference_graph(self):
        """multi_ke.py:604-621"""
        self.ckga_attribute_loss = "sum w softplus(|av - cnn|^2)"
        self._cnn_ckga = ops.multike_net(self._cnn_variables(self._dev), self.av_ent_embeds.var, self._ws_av, self.kgs.attributes_num,
                                         weighted=True)

    def _define_common_space_learning_graph(self):
        """multi_ke.py:625-638"""
        a = self.args
        self.cross_name_loss = "|f - name|^2 + |f - rv|^2 + |f - av|^2"
        self._itc_f = self._cfg(a.ITC_learning_rate, False)
        self._itc_rv = self._cfg(a.ITC_learning_rate, True)
        self._itc_av = self._cfg(a.ITC_learning_rate, False)
        self._entity_list = ops.to_ids(np.asarray(self.kgs.kg1.entities_list + self.kgs.kg2.entities_list, np.int32), self._dev)

    # ---- steps -------------------------------------------------------------------------------------------------------------------
    def _apply(self, table, rel, cfg, ws, pos=None, neg=None):
        ops.triple_step(table.var, None, rel, None, self.args.dim, self._empty if pos is None else pos, neg, cfg, ws, self._sink,
                        phase=ops.PHASE_APPLY)

    def _apply_f(self, cfg=None):
        self._apply(self.ent_embeds, self._dummy_rel, cfg or self._f_cfg, self._ws_f)

    def _apply_av(self, cfg=None):
        self._apply(self.av_ent_embeds, self.attr_embeds.var, cfg or self._av_cfg, self._ws_av)

    def _pull_names(self, ids, coef):
        ops.multike_rows(ops.MULTIKE_ROWS_PULL, self.ent_embeds.var, self._ws_f, 1, self.name_embeds.var, None, 1, None, self.args.dim,
                         ids, coef, self._loss, b_l2_norm=False)

    def _pop(self, name, trained):
        loss = float(self._loss.item())
        self._loss.zero_()
        self._sink.zero_()
        loss = loss / max(trained, 1)
        self.history.setdefault(name, []).append(loss)
        return loss

    def _sample(self, table, batch_size):
        idx = ops.sample_distinct(table.shape[0], batch_size, self._seed + 5, self._draws, dev=self._dev)
        self._draws += 1
        return table[idx.long()].contiguous()

    def train_relation_view_1epo(self, epoch, triple_steps, steps_tasks=None, batch_queue=None, neighbors1=None, neighbors2=None):
        """multi_ke.py:661-687: per batch the engine's logistic gradients, the four cross-view terms on the positives at the pre-step
        values, then both tables apply"""
        start = time.time()
        d, R = self.args.dim, self.kgs.relations_num
        f, rv, rel = self.ent_embeds.var, self.rv_ent_embeds.var, self.rel_embeds.var
        trained = 0
        for s in range(triple_steps):
            pos, neg = self._rel_epochs.batch(s)
            if pos.shape[0] == 0:
                continue
            ops.triple_step(rv, None, rel, None, d, pos, neg, self._rv_cfg, self._ws_rv, self._loss, phase=ops.PHASE_GRAD)
            ops.multike_rows(ops.MULTIKE_ROWS_CROSS, f, self._ws_f, 1, rv, self._ws_rv, R, rel, d, pos, 1.0, self._loss, rel_side=1)
            ops.multike_rows(ops.MULTIKE_ROWS_CROSS, rv, self._ws_rv, R, f, self._ws_f, 1, rel, d, pos, 1.0, self._loss, rel_side=0)
            self._pull_names(pos[:, 0].contiguous(), 0.5)
            self._pull_names(pos[:, 2].contiguous(), 0.5)
            ops.triple_step(rv, None, rel, None, d, pos, neg, self._rv_cfg, self._ws_rv, self._loss, phase=ops.PHASE_APPLY)
            self._apply_f()
            trained += pos.shape[0]
        self._rel_epochs.end_epoch()
        epoch_loss = self._pop('relation', trained)
        print('epoch {} of rel. view, avg. loss: {:.4f}, time: {:.4f}s'.format(epoch, epoch_loss, time.time() - start))

    def train_attribute_view_1epo(self, epoch, triple_steps, steps_tasks=None, batch_queue=None, neighbors1=None, neighbors2=None):
        """multi_ke.py:689-715"""
        start = time.time()
        a = self.args
        n1, n2 = self._attr_n
        if self._attr_layout is None or self._attr_layout[0] != triple_steps:
            slot, offsets = attribute_batch_layout(n1, n2, a.attribute_batch_size, triple_steps)
            self._attr_layout = (triple_steps, torch.from_numpy(slot).to(self._dev), offsets,
                                 torch.empty((len(slot), 3), dtype=torch.int32, device=self._dev))
        _, slot, offsets, dall = self._attr_layout
        self._attr_epochs += 1
        trained = 0
        if slot.numel():
            self._layout_ws = ops.epoch_layout(self._attr_all, n1, n2, slot, self._seed + 2, self._attr_epochs, dall,
                                               getattr(self, "_layout_ws", None))
        for s in range(triple_steps):
            batch = dall[int(offsets[s]):int(offsets[s + 1])]
            if batch.shape[0] == 0:
                continue
            ops.multike_cnn_step([self._cnn_av, self._cnn_f], self.attr_embeds.var, self.literal_embeds.var, a.dim, batch, self._attr_w,
                                 a.learning_rate, self._cnn_ws, self._loss)
            self._pull_names(batch[:, 0].contiguous(), 0.5)
            self._apply_av()
            self._apply_f()
            trained += batch.shape[0]
        epoch_loss = self._pop('attribute', trained)
        print('epoch {} of att. view, avg. loss: {:.4f}, time: {:.4f}s'.format(epoch, epoch_loss, time.time() - start))

    def _sampled_steps(self, n, batch_size):
        steps = int(math.ceil(n / batch_size))
        return steps, (batch_size if steps > 1 else n)

    def train_cross_kg_entity_inference_relation_view_1epo(self, epoch, sup_triples=None):
        """multi_ke.py:719-739"""
        n = self._ckge_rel.shape[0]
        if n == 0:
            return
        start = time.time()
        steps, batch_size = self._sampled_steps(n, self.args.batch_size)
        for _ in range(steps):
            pos = self._sample(self._ckge_rel, batch_size)
            ops.triple_step(self.rv_ent_embeds.var, None, self.rel_embeds.var, None, self.args.dim, pos, None, self._ckge_rel_cfg,
                            self._ws_rv, self._loss)
        epoch_loss = 2.0 * self._pop('ckge_relation', steps * batch_size)
        self.history['ckge_relation'][-1] = epoch_loss
        print('epoch {} of cross-kg entity inference in rel. view, avg. loss: {:.4f}, time: {:.4f}s'.format(epoch, epoch_loss,
                                                                                                            time.time() - start))

    def _cnn_one_net_epoch(self, name, net, triples, weights):
        n = triples.shape[0]
        steps, batch_size = self._sampled_steps(n, self.args.attribute_batch_size)
        for _ in range(steps):
            batch = self._sample(triples, batch_size)
            ops.multike_cnn_step([net], self.attr_embeds.var, self.literal_embeds.var, self.args.dim, batch, weights,
                                 self.args.learning_rate, self._cnn_ws, self._loss)
            self._apply_av()
        return self._pop(name, steps * batch_size)

    def train_cross_kg_entity_inference_attribute_view_1epo(self, epoch, sup_triples=None):
        """multi_ke.py:741-761"""
        if self._ckge_attr.shape[0] == 0:
            return
        start = time.time()
        epoch_loss = self._cnn_one_net_epoch('ckge_attribute', self._cnn_ckge, self._ckge_attr, None)
        print('epoch {} of cross-kg entity inference in attr. view, avg. loss: {:.4f}, time: {:.4f}s'.format(epoch, epoch_loss,
                                                                                                             time.time() - start))

    def train_cross_kg_relation_inference_1epo(self, epoch, sup_triples=None):
        """multi_ke.py:763-784"""
        n = self._ckgp_rel.shape[0]
        if n == 0:
            return
        start = time.time()
        rv, R = self.rv_ent_embeds.var, self.kgs.relations_num
        steps, batch_size = self._sampled_steps(n, self.args.batch_size)
        for _ in range(steps):
            pos = self._sample(self._ckgp_rel, batch_size)
            ops.multike_rows(ops.MULTIKE_ROWS_WSOFT, rv, self._ws_rv, R, rv, self._ws_rv, R, self.rel_embeds.var, self.args.dim, pos, 2.0,
                             self._loss, rel_weight=self._sup_rel_w, rel_side=0)
            self._apply(self.rv_ent_embeds, self.rel_embeds.var, self._ckgp_cfg, self._ws_rv)
        epoch_loss = self._pop('ckgp_relation', steps * batch_size)
        print('epoch {} of cross-kg relation inference in rel. view, avg. loss: {:.4f}, time: {:.4f}s'.format(epoch, epoch_loss,
                                                                                                              time.time() - start))

    def train_cross_kg_attribute_inference_1epo(self, epoch, sup_triples=None):
        """multi_ke.py:786-806"""
        if self._ckga_attr.shape[0] == 0:
            return
        start = time.time()
        epoch_loss = self._cnn_one_net_epoch('ckga_attribute', self._cnn_ckga, self._ckga_attr, self._sup_attr_w)
        print('epoch {} of cross-kg attribute inference in attr. view, avg. loss: {:.4f}, time: {:.4f}s'
              .format(epoch, epoch_loss, time.time() - start))

    def train_common_space_learning_1epo(self, epoch, entities=None):
        """multi_ke.py:827-842: all three entity tables move under ITC_learning_rate"""
        start = time.time()
        a, d = self.args, self.args.dim
        f, R, A = self.ent_embeds.var, self.kgs.relations_num, self.kgs.attributes_num
        steps, batch_size = self._sampled_steps(self._entity_list.shape[0], a.entity_batch_size)
        for _ in range(steps):
            ids = self._sample(self._entity_list, batch_size)
            self._pull_names(ids, a.cv_weight)
            ops.multike_rows(ops.MULTIKE_ROWS_PULL, f, self._ws_f, 1, self.rv_ent_embeds.var, self._ws_rv, R, None, d, ids, a.cv_weight,
                             self._loss)
            ops.multike_rows(ops.MULTIKE_ROWS_PULL, f, self._ws_f, 1, self.av_ent_embeds.var, self._ws_av, A, None, d, ids, a.cv_weight,
                             self._loss)
            self._apply_f(self._itc_f)
            self._apply(self.rv_ent_embeds, self.rel_embeds.var, self._itc_rv, self._ws_rv)
            self._apply_av(self._itc_av)
        epoch_loss = self._pop('common_space', steps * batch_size)
        if a.cv_weight:
            epoch_loss /= a.cv_weight
            self.history['common_space'][-1] = epoch_loss
        print('epoch {} of common space learning, avg. loss: {:.4f}, time: {:.4f}s'.format(epoch, epoch_loss, time.time() - start))

    def run(self):
        """multi_ke.py:844-929"""
        t = time.time()
        a, kgs = self.args, self.kgs
        relation_triples_num = kgs.kg1.local_relation_triples_num + kgs.kg2.local_relation_triples_num
        attribute_triples_num = kgs.kg1.local_attribute_triples_num + kgs.kg2.local_attribute_triples_num
        relation_triple_steps = int(math.ceil(relation_triples_num / a.batch_size))
        attribute_triple_steps = int(math.ceil(attribute_triples_num / a.batch_size))     # batch_size, as the reference has it
        self.history['nv'] = [valid_temp(self, embed_choice='nv')]
        for i in range(1, a.max_epoch + 1):
            print('epoch {}:'.format(i))
            self.train_relation_view_1epo(i, relation_triple_steps)
            self.train_common_space_learning_1epo(i)
            self.train_cross_kg_entity_inference_relation_view_1epo(i)
            if i > a.start_predicate_soft_alignment:
                self.train_cross_kg_relation_inference_1epo(i)
            self.train_attribute_view_1epo(i, attribute_triple_steps)
            self.train_common_space_learning_1epo(i)
            self.train_cross_kg_entity_inference_attribute_view_1epo(i)
            if i > a.start_predicate_soft_alignment:
                self.train_cross_kg_attribute_inference_1epo(i)
            if i >= a.start_valid and i % a.eval_freq == 0:
                valid_temp(self, embed_choice='rv')
                valid_temp(self, embed_choice='av')
                flag = self.valid(a.stop_metric)
                self.flag1, self.flag2, self.early_stop = early_stop(self.flag1, self.flag2, flag)
                if self.early_stop or i == a.max_epoch:
                    break
            if i >= a.start_predicate_soft_alignment and i % 10 == 0:
                pm = self.predicate_align_model
                pm.update_predicate_alignment(self.rel_embeds.eval())
                pm.update_predicate_alignment(self.attr_embeds.eval(), predicate_type='attribute')
                self._upload_weights()
        self._rel_epochs.check()
        print("Training ends. Total time = {:.3f} s.".format(time.time() - t))
