"""SEA (mirror of openea/approaches/sea.py:19-161): margin-based TransE pairs under Adam + two d x d mapping matrices trained
on the labelled links in both directions and, through the cycle M1 M2 / M2 M1, on the unlabelled (test + valid) links.
The mapping step is the fused oea_sea_mapping_step (csrc/sea_mapping.hip); its block normalisation is the reference's
`tf.nn.l2_normalize` without an axis (sea.py:84-92), kept as it is."""
import math
import time

import numpy as np
import torch

from .. import ops
from ..models.basic_model import BasicModel
from ..models.trainer import TripleTrainer
from ..modules.base.initializers import orthogonal_host
from ..modules.base.losses import get_loss_func
from ..modules.finding.evaluation import early_stop
from ..modules.load import read as rd
from ..modules.utils.util import task_divide


class SEA(BasicModel):

    def __init__(self):
        super().__init__()
        self.mapping_mat_1 = None
        self.mapping_mat_2 = None

    def init(self):
        self._check_device_path()
        self._check_args()
        self._define_variables()
        self._define_embed_graph()

    def _check_args(self):
        # customize parameters (sea.py:31-40)
        assert self.args.loss == 'margin-based'
        assert self.args.alignment_module == 'mapping'
        assert self.args.loss == 'margin-based'
        assert self.args.neg_sampling == 'uniform'
        assert self.args.optimizer == 'Adam'
        assert self.args.eval_metric == 'inner'
        assert self.args.loss_norm == 'L2'
        assert self.args.ent_l2_norm is True
        assert self.args.rel_l2_norm is True
        assert self.args.neg_triple_num == 1

    def _check_device_path(self):
        """the limits of the mapping step, raised before any table is made"""
        if self._dist_group() is not None:
            raise NotImplementedError("SEA runs on one GPU: the block-wide scalars of its mapping step would need an all-reduce "
                                      "between the phases of every step (launch it without torch.distributed, or with one rank)")
        if self.args.dim > ops.SEA_MAX_DIM:
            raise NotImplementedError("SEA: dim %d > %d (the mapping step holds a row in two columns per lane of one wave)"
                                      % (self.args.dim, ops.SEA_MAX_DIM))

    def _define_variables(self):
        """sea.py:42-52"""
        super()._define_variables()
        d = self.args.dim
        dev = self.ent_embeds.var.device
        rng = np.random.RandomState(self._seed + 17)
        self.mapping_mat_1 = torch.from_numpy(orthogonal_host(rng, (d, d))).to(dev)
        self.mapping_mat_2 = torch.from_numpy(orthogonal_host(rng, (d, d))).to(dev)
        self.mapping_mat = self.mapping_mat_1              # valid / test / predict map KG1's side with M1 (sea.py:100-115)
        self.eye_mat_1 = self.eye_mat_2 = self.eye_mat = torch.eye(d, dtype=torch.float32, device=dev)

    def _define_embed_graph(self):
        """sea.py:54-98: get_loss_func + Adam on the triples; a second, independent Adam instance on the mapping loss (its own
        moments of the entity table and of M1 / M2, its own step count; rel_embeds has no gradient there)."""
        self.triple_loss = get_loss_func(self.args)
        cfg, opt = self._step_cfg(self.triple_loss, 0)
        self.triple_optimizer = cfg
        self._trainer = TripleTrainer(self.ent_embeds, self.rel_embeds, cfg, opt)
        self.mapping_loss = ("alpha_1 (|L2 - gl2n(L1 M1)|^2 + |L1 - gl2n(L2 M2)|^2) + "
                             "alpha_2 (|U1 - gl2n(U1 M1 M2)|^2 + |U2 - gl2n(U2 M2 M1)|^2)")
        mcfg, mopt = self._step_cfg(dict(loss='positive', loss_norm='L2'), 0)
        self.mapping_optimizer = mcfg
        self._mapping_trainer = TripleTrainer(self.ent_embeds, self.rel_embeds, mcfg, mopt, replicated=True)
        d = self.args.dim
        self._mapping_state = (torch.zeros((4, d, d), dtype=torch.float32, device=self.ent_embeds.var.device)
                               if mopt == 'Adam' else None)              # Adam's m1, v1, m2, v2

    def _eval_valid_embeddings(self):
        if len(self.kgs.valid_links) > 0:
            embeds1 = self._lookup(self.kgs.valid_entities1)
            embeds2 = self._lookup(self.kgs.valid_entities2 + self.kgs.test_entities2)
        else:
            embeds1 = self._lookup(self.kgs.test_entities1)
            embeds2 = self._lookup(self.kgs.test_entities2)
        return embeds1, embeds2, self.mapping_mat_1

    def _eval_test_embeddings(self):
        embeds1 = self._lookup(self.kgs.test_entities1)
        embeds2 = self._lookup(self.kgs.test_entities2)
        return embeds1, embeds2, self.mapping_mat_1

    def save(self):
        """sea.py:117-123"""
        ent_embeds = self.ent_embeds.eval()
        rel_embeds = self.rel_embeds.eval()
        rd.save_embeddings(self.out_folder, self.kgs, ent_embeds, rel_embeds, None, mapping_mat=self.mapping_mat_1.cpu().numpy(),
                           rev_mapping_mat=self.mapping_mat_2.cpu().numpy())

    def launch_training_1epo(self, epoch, triple_steps, steps_tasks, training_batch_queue, neighbors1, neighbors2):
        self.launch_triple_training_1epo(epoch, triple_steps, steps_tasks, training_batch_queue, neighbors1, neighbors2)
        self.launch_mapping_training_1epo(epoch, triple_steps)

    def _draw(self, links, n_batch, steps, gen):
        """random.sample(links, n_batch) per step = the first n_batch of a random permutation, for all steps at once on the
        device -> [steps, 2, n_batch] (side 1 row, side 2 row)"""
        if n_batch == 0:
            return torch.zeros((steps, 2, 0), dtype=torch.int32, device=links.device)
        picks = torch.rand((steps, links.shape[0]), device=links.device, generator=gen).argsort(dim=1)[:, :n_batch]
        return links[picks.reshape(-1)].reshape(steps, n_batch, 2).permute(0, 2, 1)

    def launch_mapping_training_1epo(self, epoch, triple_steps):
        """sea.py:129-145: triple_steps steps on |train| // steps labelled and |test + valid| // steps unlabelled links each;
        ONE C call enqueues the epoch (oea_sea_mapping_epoch)."""
        start = time.time()
        dev = self.mapping_mat_1.device
        if getattr(self, "_labelled_dev", None) is None:
            self._labelled_dev = ops.to_ids(np.asarray(self.kgs.train_links, np.int32).reshape(-1, 2), dev)
            self._unlabelled_dev = ops.to_ids(np.asarray(list(self.kgs.test_links) + list(self.kgs.valid_links),
                                                         np.int32).reshape(-1, 2), dev)
        n_l = self._labelled_dev.shape[0] // triple_steps
        n_u = self._unlabelled_dev.shape[0] // triple_steps
        gen = torch.Generator(device=dev)
        gen.manual_seed(self._seed + 1000 + epoch)
        lab = self._draw(self._labelled_dev, n_l, triple_steps, gen)
        unl = self._draw(self._unlabelled_dev, n_u, triple_steps, gen)
        batches = torch.cat([lab.reshape(triple_steps, 2 * n_l), unl.reshape(triple_steps, 2 * n_u)], dim=1).contiguous()
        t = self._mapping_trainer
        loss_dev = torch.zeros(1, dtype=torch.float64, device=dev)
        t.count_steps(triple_steps)
        self._mapping_work = ops.sea_mapping_epoch(self.ent_embeds.var, t.ent_acc, self.rel_embeds.var, t.rel_acc, self.args.dim,
                                                   batches, n_l, n_u, self.mapping_mat_1, self.mapping_mat_2, self._mapping_state,
                                                   float(self.args.alpha_1), float(self.args.alpha_2), t.cfg, t.ws, loss_dev,
                                                   t.loss, getattr(self, "_mapping_work", None))
        trained_samples_num = n_l * triple_steps
        epoch_loss = float(loss_dev.item()) / max(trained_samples_num, 1)
        print('epoch {}, avg. mapping loss: {:.4f}, cost time: {:.4f}s'.format(epoch, epoch_loss, time.time() - start))

    def run(self):
        """sea.py:147-161"""
        t = time.time()
        triples_num = self.kgs.kg1.relation_triples_num + self.kgs.kg2.relation_triples_num
        triple_steps = int(math.ceil(triples_num / self.args.batch_size))
        steps_tasks = task_divide(list(range(triple_steps)), self.args.batch_threads_num)
        for i in range(1, self.args.max_epoch + 1):
            self.launch_training_1epo(i, triple_steps, steps_tasks, None, None, None)
            if i >= self.args.start_valid and i % self.args.eval_freq == 0:
                flag = self.valid(self.args.stop_metric)
                self.flag1, self.flag2, self.early_stop = early_stop(self.flag1, self.flag2, flag)
                if self.early_stop or i == self.args.max_epoch:
                    break
        if self._epochs is not None:
            self._epochs.check()
        print("Training ends. Total time = {:.3f} s.".format(time.time() - t))
