"""MultiKE's predicate alignment (mirror of openea/approaches/predicate_alignmnet.py, the module name misspelt as there).

The name ratios of init_predicate_alignment are Levenshtein.ratio in the reference; here one oea_lcs_ratio_pairs call
(csrc/lcs_sim.hip: 2 LCS / (|a| + |b|), the same number) gives all |P1| x |P2| of them and the selection runs on the host.
find_predicate_alignment_by_embedding stays on the host: a few hundred rows every ten epochs.

Deliberate differences:
  * ORDER.  The reference iterates dicts built from sets of URI strings and returns `list(set)`: both change with PYTHONHASHSEED.
    Here predicates are walked in sorted order (a tie between two names goes to the smaller URI) and every list is sorted.
  * WEIGHT VECTORS.  In add_weights and generate_sup_predicate_triples the weight of a triple is a function of its predicate id
    alone (links are one to one: link2dic asserts it), so next to the reference's weighted triple lists the model keeps one float
    vector per predicate table (weight_vector, sup_weight_vector) and the device steps read that."""
import numpy as np


def link2dic(links):
    dic1, dic2 = dict(), dict()
    for i, j, w in links:
        dic1[i] = (j, w)
        dic2[j] = (i, w)
    assert len(dic1) == len(dic2)
    return dic1, dic2


def generate_sup_predicate_triples(predicate_links, triples1, triples2):
    link_dic1, link_dic2 = link2dic(predicate_links)
    sup_triples1, sup_triples2 = set(), set()
    for s, p, o in triples1:
        if p in link_dic1:
            sup_triples1.add((s, link_dic1.get(p)[0], o, link_dic1.get(p)[1]))
    for s, p, o in triples2:
        if p in link_dic2:
            sup_triples2.add((s, link_dic2.get(p)[0], o, link_dic2.get(p)[1]))
    return sorted(sup_triples1), sorted(sup_triples2)


def zoom_weight(weight, min_w_before, min_w_after=0.5):
    weight_new = 1.0 - (1.0 - weight) * (1.0 - min_w_after) / (1.0 - min_w_before)
    return weight_new


def add_weights(predicate_links, triples1, triples2, min_w_before):
    link_dic1, link_dic2 = link2dic(predicate_links)
    weighted_triples1, weighted_triples2 = set(), set()
    w = 0.2
    for s, p, o in triples1:
        if p in link_dic1:
            weighted_triples1.add((s, p, o, zoom_weight(link_dic1.get(p)[1], min_w_before)))
        else:
            weighted_triples1.add((s, p, o, w))
    for s, p, o in triples2:
        if p in link_dic2:
            weighted_triples2.add((s, p, o, zoom_weight(link_dic2.get(p)[1], min_w_before)))
        else:
            weighted_triples2.add((s, p, o, w))
    assert len(triples1) == len(weighted_triples1)
    assert len(triples2) == len(weighted_triples2)
    return sorted(weighted_triples1), sorted(weighted_triples2), weighted_triples1, weighted_triples2


def weight_vector(predicate_links, predicates1, predicates2, n_predicates, min_w_before):
    """add_weights as a vector over the predicate ids: 0.2, or the zoomed weight of the link a predicate of its own KG is in.
    An id that both KGs use with two different weights has no vector form: ValueError."""
    link_dic1, link_dic2 = link2dic(predicate_links)
    vec = np.full(n_predicates, 0.2, np.float64)
    seen = {}
    for dic, predicates in ((link_dic1, predicates1), (link_dic2, predicates2)):
        for p in predicates:
            w = zoom_weight(dic[p][1], min_w_before) if p in dic else 0.2
            if seen.setdefault(p, w) != w:
                raise ValueError("predicate id %d carries the weights %r and %r in the two KGs" % (p, seen[p], w))
            vec[p] = w
    return vec


def sup_weight_vector(predicate_links, n_predicates):
    """generate_sup_predicate_triples' weights over the ids of the predicates that are swapped IN: the link's weight"""
    vec = np.zeros(n_predicates, np.float64)
    for i, j, w in predicate_links:
        for p in (i, j):
            if vec[p] not in (0.0, w):
                raise ValueError("predicate id %d is swapped in with two weights" % p)
            vec[p] = w
    return vec


def plain_ratio(a, b):
    """2 LCS / (|a| + |b|) on the host (Levenshtein.ratio's number, the one oea_lcs_ratio_pairs returns); 1.0 for two empty strings"""
    if not a and not b:
        return 1.0
    prev = [0] * (len(b) + 1)
    for ca in a:
        cur = [0]
        for j, cb in enumerate(b):
            cur.append(prev[j] + 1 if ca == cb else max(prev[j + 1], cur[j]))
        prev = cur
    return 2.0 * prev[-1] / (len(a) + len(b))


def name_ratios(names1, names2, on_device=True):
    """-> float64 [len(names1), len(names2)]"""
    if not names1 or not names2:
        return np.zeros((len(names1), len(names2)))
    if not on_device:
        return np.array([[plain_ratio(a, b) for b in names2] for a in names1])
    from .. import ops
    pool1, pool2 = ops.StringPool(names1), ops.StringPool(names2)
    pairs = np.stack(np.meshgrid(pool1.ids(names1), pool2.ids(names2), indexing='ij'), -1).reshape(-1, 2)
    _, ratio = ops.lcs_ratio_pairs(pool1, pool2, ops.to_ids(pairs, pool1.cp.device))
    return ratio.cpu().numpy().astype(np.float64).reshape(len(names1), len(names2))


def init_predicate_alignment(predicate_local_name_dict_1, predicate_local_name_dict_2, predicate_init_sim, ratios=None):
    """predicate_alignmnet.py:46-72 over the ratio matrix of the two name lists in sorted key order (computed on the device when
    `ratios` is None) -> (pairs (p1, p2, sim) above predicate_init_sim, {(p1, p2): sim} of every mutual best match)"""
    keys1, keys2 = sorted(predicate_local_name_dict_1), sorted(predicate_local_name_dict_2)
    if ratios is None:
        ratios = name_ratios([predicate_local_name_dict_1[k] for k in keys1], [predicate_local_name_dict_2[k] for k in keys2])

    def get_predicate_match_dict(ks1, ks2, sim):
        predicate_match_dict, sim_dict = {}, {}
        for i, p1 in enumerate(ks1):
            match_p2 = ''
            max_sim = 0
            for j, p2 in enumerate(ks2):
                if sim[i, j] > max_sim:
                    match_p2 = p2
                    max_sim = float(sim[i, j])
            predicate_match_dict[p1] = match_p2
            sim_dict[p1] = max_sim
        return predicate_match_dict, sim_dict

    match_dict_1_2, sim_dict_1 = get_predicate_match_dict(keys1, keys2, ratios)
    match_dict_2_1, _ = get_predicate_match_dict(keys2, keys1, ratios.T)
    predicate_match_pairs_set = set()
    predicate_latent_match_pairs_similarity_dict = {}
    for p1, p2 in match_dict_1_2.items():
        if p2 in match_dict_2_1 and match_dict_2_1[p2] == p1:
            predicate_latent_match_pairs_similarity_dict[(p1, p2)] = sim_dict_1[p1]
            if sim_dict_1[p1] > predicate_init_sim:
                predicate_match_pairs_set.add((p1, p2, sim_dict_1[p1]))
    return predicate_match_pairs_set, predicate_latent_match_pairs_similarity_dict


def predicate2id_matched_pairs(predicate_match_pairs_set, predicate_id_dict_1, predicate_id_dict_2):
    id_match_pairs_set = set()
    for (p1, p2, w) in predicate_match_pairs_set:
        if p1 in predicate_id_dict_1 and p2 in predicate_id_dict_2:
            id_match_pairs_set.add((predicate_id_dict_1[p1], predicate_id_dict_2[p2], w))
    return id_match_pairs_set


def find_predicate_alignment_by_embedding(embed, predicate_list1, predicate_list2, predicate_id_dict1=None, predicate_id_dict2=None):
    """predicate_alignmnet.py:97-126: mutual nearest neighbours under the cosine of the rows -> {(i, j): similarity}"""
    embed = np.asarray(embed, np.float64)
    norm = np.linalg.norm(embed, axis=1, keepdims=True)
    embed = embed / np.where(norm == 0, 1.0, norm)                       # sklearn.preprocessing.normalize
    sim_mat = np.matmul(embed, embed.T)
    set1, set2 = set(predicate_list1), set(predicate_list2)
    matched_1, matched_2 = {}, {}
    for i in predicate_list1:
        for j in (-sim_mat[i, :]).argsort(kind='stable'):
            if j in set2:
                matched_1[i] = int(j)
                break
    for j in predicate_list2:
        for i in (-sim_mat[j, :]).argsort(kind='stable'):
            if i in set1:
                matched_2[j] = int(i)
                break
    out = {}
    for i, j in matched_1.items():
        if matched_2[j] == i:
            out[(i, j)] = float(sim_mat[i, j])
    return out


def get_local_name(item_set):
    item_local_name_dict = {}
    for item in item_set:
        item_local_name_dict[item] = item.split('/')[-1].replace('_', ' ')
    return item_local_name_dict


class PredicateAlignModel:
    def __init__(self, kgs, args):
        self.kgs = kgs
        self.args = args
        self.relation_name_dict1 = get_local_name(set(self.kgs.kg1.relations_id_dict.keys()))
        self.attribute_name_dict1 = get_local_name(set(self.kgs.kg1.attributes_id_dict.keys()))
        self.relation_name_dict2 = get_local_name(set(self.kgs.kg2.relations_id_dict.keys()))
        self.attribute_name_dict2 = get_local_name(set(self.kgs.kg2.attributes_id_dict.keys()))
        self.relation_alignment_set, self.relation_latent_match_pairs_similarity_dict_init = \
            init_predicate_alignment(self.relation_name_dict1, self.relation_name_dict2, self.args.predicate_init_sim)
        self.attribute_alignment_set, self.attribute_latent_match_pairs_similarity_dict_init = \
            init_predicate_alignment(self.attribute_name_dict1, self.attribute_name_dict2, self.args.predicate_init_sim)
        self.relation_alignment_set_init = self.relation_alignment_set
        self.attribute_alignment_set_init = self.attribute_alignment_set
        self.update_relation_triples(self.relation_alignment_set)
        self.update_attribute_triples(self.attribute_alignment_set)

    def update_attribute_triples(self, attribute_alignment_set):
        kg1, kg2 = self.kgs.kg1, self.kgs.kg2
        self.attribute_id_alignment_set = predicate2id_matched_pairs(attribute_alignment_set, kg1.attributes_id_dict, kg2.attributes_id_dict)
        links = sorted(self.attribute_id_alignment_set)
        self.train_attributes1 = [a for (a, _, _) in links]
        self.train_attributes2 = [a for (_, a, _) in links]
        self.sup_attribute_alignment_triples1, self.sup_attribute_alignment_triples2 = \
            generate_sup_predicate_triples(links, kg1.local_attribute_triples_list, kg2.local_attribute_triples_list)
        self.attribute_triples_w_weights1, self.attribute_triples_w_weights2, self.attribute_triples_w_weights_set1, \
            self.attribute_triples_w_weights_set2 = add_weights(links, kg1.local_attribute_triples_list, kg2.local_attribute_triples_list,
                                                                self.args.predicate_soft_sim)
        self.attribute_weights = weight_vector(links, kg1.attributes_list, kg2.attributes_list, self.kgs.attributes_num,
                                               self.args.predicate_soft_sim)
        self.sup_attribute_weights = sup_weight_vector(links, self.kgs.attributes_num)

    def update_relation_triples(self, relation_alignment_set):
        kg1, kg2 = self.kgs.kg1, self.kgs.kg2
        self.relation_id_alignment_set = predicate2id_matched_pairs(relation_alignment_set, kg1.relations_id_dict, kg2.relations_id_dict)
        links = sorted(self.relation_id_alignment_set)
        self.train_relations1 = [a for (a, _, _) in links]
        self.train_relations2 = [a for (_, a, _) in links]
        self.sup_relation_alignment_triples1, self.sup_relation_alignment_triples2 = \
            generate_sup_predicate_triples(links, kg1.local_relation_triples_list, kg2.local_relation_triples_list)
        self.relation_triples_w_weights1, self.relation_triples_w_weights2, self.relation_triples_w_weights_set1, \
            self.relation_triples_w_weights_set2 = add_weights(links, kg1.local_relation_triples_list, kg2.local_relation_triples_list,
                                                               self.args.predicate_soft_sim)
        self.relation_weights = weight_vector(links, kg1.relations_list, kg2.relations_list, self.kgs.relations_num,
                                              self.args.predicate_soft_sim)
        self.sup_relation_weights = sup_weight_vector(links, self.kgs.relations_num)

    def update_predicate_alignment(self, embed, predicate_type='relation', w=0.7):
        if predicate_type == 'relation':
            predicate_list1, predicate_list2 = self.kgs.kg1.relations_list, self.kgs.kg2.relations_list
            predicate_id_dict1, predicate_id_dict2 = self.kgs.kg1.relations_id_dict, self.kgs.kg2.relations_id_dict
            predicate_alignment_set_init = self.relation_alignment_set_init
        else:
            predicate_list1, predicate_list2 = self.kgs.kg1.attributes_list, self.kgs.kg2.attributes_list
            predicate_id_dict1, predicate_id_dict2 = self.kgs.kg1.attributes_id_dict, self.kgs.kg2.attributes_id_dict
            predicate_alignment_set_init = self.attribute_alignment_set_init
        latent = find_predicate_alignment_by_embedding(embed, predicate_list1, predicate_list2, predicate_id_dict1, predicate_id_dict2)
        predicate_alignment_set = set()
        for (p1, p2, sim_init) in sorted(predicate_alignment_set_init):
            p_id_1 = predicate_id_dict1[p1]
            p_id_2 = predicate_id_dict2[p2]
            sim = sim_init
            if (p_id_1, p_id_2) in latent:
                sim = w * sim + (1 - w) * latent[(p_id_1, p_id_2)]
            if sim > self.args.predicate_soft_sim:
                predicate_alignment_set.add((p1, p2, sim))
        print('update ' + predicate_type + ' alignment:', len(predicate_alignment_set))
        if predicate_type == 'relation':
            self.relation_alignment_set = predicate_alignment_set
            self.update_relation_triples(predicate_alignment_set)
        else:
            self.attribute_alignment_set = predicate_alignment_set
            self.update_attribute_triples(predicate_alignment_set)
