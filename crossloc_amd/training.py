"""Training library for the two training entry points (train_single_task.py, finetune_decoder_single_task.py).

Reference: utils/learning.py:84-175 (label means), :266-398 (config_network), train_single_task.py:207-326 (loop).
  config_network   builds the TransPoseNet of a task with the reference's rules (channels, MLR encoders loaded from
                   their checkpoints and frozen, decoder initialised from the coord checkpoint); host only.
  make_step        one iteration (forward, uncertainty split, fused loss, backward, gradient all-reduce, fused Adam) as
                   HIP launches plus at most one collective; returns device scalars, nothing synchronises.
  make_e2e_step    its sibling for end-to-end DSAC* training (train_e2e.py): forward, the solver's backward pass and the
                   finishing op in place of the fused loss, [joined with the coord loss,] then the same tail.
  epoch_batches    the data-parallel sampler: one seeded permutation per epoch, identical on every rank, cut into
                   disjoint per-rank shards.
  Trainer          the loop: schedule, reference checkpoints (model.net, ckpt_iter_%07d.net, FLAG_training_done.nodata)
                   and resume.pt (optimiser, scheduler, counters, sampler position, RNG states).
"""
import collections
import logging
import math
import os
import random
import time

import numpy as np
import torch

from . import loss as xl_loss
from . import networks, optim, switches

TASK_CHANNELS = {'coord': 3, 'depth': 1, 'normal': 2, 'semantics': 6}     # learning.py:273-283
SAMPLER_SEED = 2021
# the distributed switch of the driver: several ranks on cuda:0, gradients reduced through gloo on a host copy
SHARED_GPU_ENV = "XL_TRAIN_SHARED_GPU"


def set_random_seed(random_seed):
    """utils/learning.py:74-81"""
    torch.manual_seed(random_seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(random_seed)
    random.seed(random_seed)
    np.random.seed(random_seed)


def _known_scene(scene):
    s = scene.lower()
    return 'urbanscape' in s or 'naturescape' in s


def get_nodata_value(scene):
    """utils/learning.py:38-46"""
    if not _known_scene(scene):
        raise NotImplementedError("scene %r: only urbanscape and naturescape scenes are known" % scene)
    return -1


def get_label_mean(scene, task):
    """The scene constants of utils/learning.py:84-175.  The reference computes the mean from the data for other scenes;
    those are not supported here (as get_nodata_value)."""
    if not _known_scene(scene):
        raise NotImplementedError("scene %r: label means are known for urbanscape and naturescape only" % scene)
    nature = 'naturescape' in scene
    if task == 'coord':
        return torch.tensor([-455.934, 417.50, 520.31] if nature else [-29.34, 184.17, 91.96]).float()
    if task == 'depth':
        return torch.tensor([241.47] if nature else [136.24]).float()
    if task == 'normal':
        mean = (torch.tensor([-0.7943, -0.9986] if nature else [-1.0454, -0.9858]) / np.pi + 1.0) / 2.0
        return (-torch.log((1 / (mean + 1.e-7)) - 1.0)).float()
    if task == 'semantics':
        return torch.zeros(6)
    raise NotImplementedError(task)


def state_dict(network):
    """`network.state_dict()` as a plain OrderedDict of tensors - the reference checkpoint format.  (The module's own
    state_dict carries per-module metadata in which TransPoseNet's `_version` method stands for nn.Module's version number;
    a file holding it does not load with torch.load's weights_only default.)"""
    from collections import OrderedDict
    return OrderedDict(network.state_dict())


def load_module(module, weights, prefix='encoder.'):
    """`_load_module` of utils/learning.py:325-333: every state_dict entry of `module` from `weights[key]`, or else from
    `weights[prefix + key]`; a missing entry is an error."""
    own = module.state_dict()
    with torch.no_grad():
        for key in own.keys():
            if key in weights:
                own[key].copy_(weights[key])
            elif prefix + key in weights:
                own[key].copy_(weights[prefix + key])
            else:
                raise KeyError("%s (or %s%s) is not in the checkpoint" % (key, prefix, key))


def config_network(task, tiny, grayscale, uncertainty, fullsize, mean, encoders_in=None, reuse_coord_encoder=False,
                   unfreeze_coord_encoder=False, network_in=None):
    """utils/learning.py:266-365 for urbanscape / naturescape scenes: the network of `task`, on the host.  `encoders_in`:
    checkpoint paths, the coord network's first (its decoder initialises this decoder; its encoder is reused when
    `reuse_coord_encoder`); the other encoders are loaded and frozen.  `network_in`: a full state_dict loaded strictly,
    which supersedes the encoder checkpoints (resume)."""
    if task not in TASK_CHANNELS:
        raise NotImplementedError(task)
    if uncertainty not in (None, 'MLE'):
        raise NotImplementedError(uncertainty)
    if task == 'semantics' and (uncertainty is not None or not fullsize):
        raise NotImplementedError("semantics needs --fullsize and no uncertainty")
    if encoders_in is None:
        num_mlr = 0
    elif reuse_coord_encoder:
        num_mlr = len(encoders_in)
    else:
        assert not unfreeze_coord_encoder
        num_mlr = len(encoders_in) - 1                   # the coord weight only initialises the decoder
    network = networks.TransPoseNet(mean, tiny, grayscale, 2, 2, TASK_CHANNELS[task], 0 if uncertainty is None else 1,
                                    32, num_mlr, 1 if unfreeze_coord_encoder else 0, fullsize)
    logging.info("{:d} network weights to load, flag_unfreeze_coord_encoder: {}".format(num_mlr, unfreeze_coord_encoder))
    if network_in is not None:
        network.load_state_dict(torch.load(network_in, map_location="cpu"), strict=True)
        logging.info("Successfully loaded %s." % network_in)
    if encoders_in is not None:
        loading = network_in is None
        enc = 0
        for i, path in enumerate(encoders_in):
            if i == 0:
                assert 'coord' in os.path.abspath(path), "the first encoder weight must be the coord network's"
                if loading:
                    load_module(network.decoder, torch.load(path, map_location="cpu"), prefix='decoder.')
                if not reuse_coord_encoder:
                    continue
            if loading:
                load_module(network.mlr_encoder_ls[enc], torch.load(path, map_location="cpu"), prefix='encoder.')
                logging.info("Loaded %s as encoder %d" % (path, enc))
            if not (i == 0 and unfreeze_coord_encoder):
                for p in network.mlr_encoder_ls[enc].parameters():
                    p.requires_grad = False
            enc += 1
        groups = [('Vanilla encoder', network.encoder_ls),
                  ('MLR encoder', list(network.mlr_encoder_ls) + [network.mlr_norm, network.mlr_forward, network.mlr_skip]),
                  ('Decoder', network.decoder_ls)]
        info, total = 'Recounting #trainable parameters: ', 0
        for name, mods in groups:
            n = sum(p.numel() for m in mods for p in m.parameters() if p.requires_grad)
            total += n
            info += '{:s}: {:,d}, '.format(name, n)
        logging.info(info + 'Total: {:,d}.'.format(total))
    return network


def allreduce_flat_gradients(network, world_size, group=None, host=False):
    """Average the gradients of `network` over the ranks with ONE all-reduce of the backward pass's flat result buffer
    (networks.gradient_buffer) - no per-step flatten / scatter.  RCCL: ReduceOp.AVG on the device buffer.  `host`
    (several ranks sharing one GPU, where RCCL refuses the group): sum through gloo on a host copy, halve there, copy back."""
    import torch.distributed as dist
    flat = networks.gradient_buffer(network)
    if host:
        h = flat.cpu()
        dist.all_reduce(h, op=dist.ReduceOp.SUM, group=group)
        h.div_(world_size)
        flat.copy_(h)
    else:
        dist.all_reduce(flat, op=dist.ReduceOp.AVG, group=group)


def make_step(network, task, optimizer, uncertainty=None, nodata_value=-1, mindepth=0.1, softclamp=100.0,
              hardclamp=1000.0, inittolerance=50.0, world_size=1, group=None, host_reduce=False):
    """One iteration of train_single_task.py:245-301 for `task`: step(images, gt_poses, gt_labels, focal_length) with
    device tensors (focal_length: a float, the first frame's as the reference uses - or one focal length per frame, a
    sequence or tensor of B, which the coord loss then applies frame by frame) -> (loss, valid_rate) device scalars."""
    if task not in TASK_CHANNELS:
        raise NotImplementedError(task)
    pixel_grid = xl_loss.get_pixel_grid(network.OUTPUT_SUBSAMPLE) if task == 'coord' else None

    def step(images, gt_poses, gt_labels, focal_length):
        predictions = network(images)
        focals = None
        if task == 'coord' and not isinstance(focal_length, (int, float)) and getattr(focal_length, 'ndim', 1) > 0:
            focals, focal_length = focal_length, 1.0       # per frame: cam_mat only supplies the principal point
        cam_mat = xl_loss.get_cam_mat(images.size(3), images.size(2), focal_length) if task == 'coord' else None
        # the loss kernel reads the output in place and writes d loss / d output whole: the uncertainty split
        # (train_single_task.py:266-271) is a channel offset, and no autograd node of the loss launches anything
        loss, rate, grad = xl_loss.task_loss_and_output_gradient(
            task, uncertainty, predictions, network.num_task_channel, gt_labels, gt_poses, pixel_grid, cam_mat,
            nodata_value, mindepth, softclamp, hardclamp, inittolerance, focals=focals)
        predictions.backward(grad)
        if world_size > 1:
            allreduce_flat_gradients(network, world_size, group, host_reduce)
        optimizer.step()
        optimizer.zero_grad(set_to_none=True)          # no view of the gradient buffer outlives the step
        return loss.detach(), rate

    return step


def e2e_keys(seed, batch, step_index):
    """(solver seed, image0) of an end-to-end step: the run's --seed plus the step index, and the dataset index of the
    batch's first frame (frame b of the batch draws as image image0 + b).  They depend on the sampler's batch and the step
    index only, so a step is reproducible wherever it runs; the solver's ABI keys a batch by such a sequence."""
    return int(seed) + int(step_index), int(batch[0])


def make_e2e_step(network, optimizer, opt, world_size=1, group=None, host_reduce=False):
    """One iteration of end-to-end DSAC* training: step(images, gt_poses, gt_labels, focals, step_index, image0=0) with device
    tensors (focals: one per frame, host or device; gt_labels: the coord labels, or a dict with 'coord' and, for --mode
    rgbd, 'depth') -> (mean expected pose loss, summary row of loss.E2E_SUMMARY_FIELDS), device tensors; nothing
    synchronises.  Forward, [the coord loss's output gradient times opt.init_weight,] the solver's backward pass and the
    finishing op added onto it, backward, gradient all-reduce, fused Adam.  `opt`: the options of train_e2e.py.  With
    opt.aug_canvas the frames carry their own scale: the coord term then reads one focal length per frame.  With
    opt.mask == 'labels' (--mode rgb) every step builds evaluation.cell_mask from its coord labels: the cells whose label is the
    scene's nodata value - sky, water, the empty border of a warped frame - are no evidence for the solver and get no pose
    gradient (dsacstar.backward_rgb_masked_batch), drawn by the sampler opt.mask_sampler names (default 'reject')"""
    rgbd = opt.mode == 'rgbd'
    label_mask = getattr(opt, 'mask', 'none') == 'labels'
    mask_sampler = getattr(opt, 'mask_sampler', 'reject')
    if mask_sampler != 'reject' and not label_mask:
        raise RuntimeError("--mask_sampler %s is the masked solver's: it needs --mask labels" % mask_sampler)
    if label_mask and rgbd:
        raise RuntimeError("--mask labels is for --mode rgb: the RGB-D solver drops depth holes itself and takes no mask")
    canvas = bool(getattr(opt, 'aug_canvas', False))
    joint = opt.init_weight > 0
    sub = network.OUTPUT_SUBSAMPLE
    pixel_grid = xl_loss.get_pixel_grid(sub) if joint else None
    nodata_value = get_nodata_value(opt.scene)

    def step(images, gt_poses, gt_labels, focals, step_index, image0=0):
        predictions = network(images)
        image_h, image_w = images.size(2), images.size(3)
        focals = torch.as_tensor(focals, dtype=torch.float32).reshape(-1)
        grad, beta = None, 0.0
        if joint:
            gt_coords = gt_labels['coord'] if isinstance(gt_labels, dict) else gt_labels
            # the first frame's focal length, as make_step; canvas mode: cam_mat's is unused, each frame has its own
            cam_mat = xl_loss.get_cam_mat(image_w, image_h, 1.0 if canvas else float(focals[0]))
            _, _, grad = xl_loss.task_loss_and_output_gradient(
                'coord', opt.uncertainty, predictions, network.num_task_channel, gt_coords, gt_poses, pixel_grid, cam_mat,
                nodata_value, opt.mindepth, opt.softclamp, opt.hardclamp, opt.inittolerance,
                focals=focals if canvas else None)
            beta = opt.init_weight
        # the depth label is -1 where nothing was measured; the RGB-D solver takes 0 for that
        depth = gt_labels['depth'][:, 0].clamp_min(0.0) if rgbd else None
        mask = None
        if label_mask:
            from .evaluation import cell_mask
            mask = cell_mask(labels=gt_labels['coord'] if isinstance(gt_labels, dict) else gt_labels, nodata_value=nodata_value)
        seed, image0 = e2e_keys(opt.seed, (image0,), step_index)     # image0: the first frame's dataset index
        loss, stats, grad = xl_loss.expected_pose_loss_and_output_gradient(
            predictions, gt_poses, focals, image_h, image_w, opt.hypotheses, opt.threshold, opt.inlieralpha,
            opt.maxpixelerror, opt.weightrot, opt.weighttrans, opt.softclamp, seed, image0=image0,
            clip_norm=opt.clip_norm, weight=1.0, grad=grad, beta=beta, depth=depth, rgbd_threshold=opt.threshold,
            max_dist_error=opt.maxpixelerror, subsample=sub, mask=mask, mask_sampler=mask_sampler)
        predictions.backward(grad)
        if world_size > 1:
            allreduce_flat_gradients(network, world_size, group, host_reduce)
        optimizer.step()
        optimizer.zero_grad(set_to_none=True)          # no view of the gradient buffer outlives the step
        return loss, stats[-1]

    return step


def epoch_batches(n, epoch, batch_size, rank=0, world_size=1, seed=SAMPLER_SEED):
    """The frames of every step of one epoch for `rank`: a permutation of range(n) seeded by (seed, epoch), the same on
    every rank, cut into `world_size` disjoint shards of n // world_size frames (the tail is dropped so that every rank
    runs the same number of steps), each split into batches of `batch_size` (the last one may be shorter)."""
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed + epoch)).tolist()
    per = n // world_size
    mine = perm[rank * per:(rank + 1) * per]
    return [mine[i:i + batch_size] for i in range(0, per, batch_size)]


def get_training_dirs(scene_dir, real_data_domain, real_data_chunk, sim_data_chunk, real_only):
    """The sections of utils/learning.py:199-230 below `scene_dir` (the reference's ./datasets/<scene>)."""
    assert real_data_domain in ('in_place', 'out_of_place'), real_data_domain
    assert 1.0 >= real_data_chunk >= 0.0 and 1.0 >= sim_data_chunk >= 0.0
    assert real_data_chunk > 0.0 or sim_data_chunk > 0.0, "one of real_data_chunk or sim_data_chunk must be positive!"
    dirs = []
    if sim_data_chunk > 0:
        dirs.append("train_sim" if sim_data_chunk == 1 else "train_sim_chunk_{:.2f}".format(sim_data_chunk))
    if real_data_chunk > 0:
        oop = "oop_" if real_data_domain == 'out_of_place' else ""
        sfx = "" if real_data_chunk == 1 else "_chunk_{:.2f}".format(real_data_chunk)
        dirs.append("train_{}drone_real{}".format(oop, sfx))
        if not real_only:
            dirs.append("train_{}drone_sim{}".format(oop, sfx))
    dirs = [os.path.join(scene_dir, d) for d in dirs]
    missing = [d for d in dirs if not os.path.isdir(d)]
    if missing:
        raise FileNotFoundError("training data directory not found: %s (sections chosen by --real_data_domain / "
                                "--real_data_chunk / --sim_data_chunk / --real_only under --scene_dir)" % ", ".join(missing))
    return dirs


def _atomic_save(obj, path):
    tmp = path + ".tmp"
    torch.save(obj, tmp)
    os.replace(tmp, path)


def resume_source(opt, output_dir):
    """The resume.pt a run continues from, or None for a fresh start.  --auto_resume (utils/io.py:114-208): the run's own
    output folder, when it holds the state of an earlier run, else a fresh start - every script line passes it, first runs
    included; --network_in is then only the initialisation of a fresh start.  --epoch_plus: the finished run whose
    model.net --network_in names, extended to --epochs in a new output folder."""
    if opt.auto_resume:
        path = os.path.join(output_dir, 'resume.pt')
        return path if os.path.exists(path) else None
    if opt.epoch_plus:
        if opt.network_in is None:
            raise ValueError("--epoch_plus needs --network_in: the model.net of the finished run to extend")
        path = os.path.join(os.path.dirname(os.path.abspath(opt.network_in)), 'resume.pt')
        if not os.path.exists(path):
            raise FileNotFoundError("--epoch_plus: %s does not exist" % path)
        return path
    return None


def _rng_state():
    st = dict(random=random.getstate(), numpy=np.random.get_state(), torch=torch.get_rng_state())
    if torch.cuda.is_available():
        st["cuda"] = torch.cuda.get_rng_state_all()
    return st


def _set_rng_state(st):
    random.setstate(st["random"])
    np.random.set_state(st["numpy"])
    torch.set_rng_state(st["torch"])
    if "cuda" in st and torch.cuda.is_available():
        torch.cuda.set_rng_state_all(st["cuda"])


class Trainer:
    """The loop of train_single_task.py:207-326 over a CamLocDataset(augment=True), data parallel over `world_size`
    ranks.  `iteration` counts frames over all ranks (the reference's counter); a de-facto epoch is len(dataset) frames.
    `e2e`: the loop takes make_e2e_step's step (end-to-end DSAC* training, `opt` from train_e2e.py) in place of make_step's;
    sampler, schedule, checkpoints and resume are the same."""

    def __init__(self, network, dataset, task, opt, output_dir, ckpt_dir, device, rank=0, world_size=1, group=None,
                 host_reduce=False, num_workers=0, e2e=False):
        self.network, self.dataset, self.task, self.opt = network, dataset, task, opt
        self.output_dir, self.ckpt_dir, self.device = output_dir, ckpt_dir, device
        self.rank, self.world_size, self.num_workers = rank, world_size, num_workers
        self.optimizer = optim.Adam(network.parameters(), lr=opt.learningrate)
        if opt.no_lr_scheduling:
            self.scheduler = torch.optim.lr_scheduler.MultiStepLR(self.optimizer, [999999], gamma=1.0)
        else:
            self.scheduler = torch.optim.lr_scheduler.MultiStepLR(self.optimizer, [50, 100], gamma=0.5)
        self.e2e = e2e
        if e2e:
            self.step_fn = make_e2e_step(network, self.optimizer, opt, world_size, group, host_reduce)
        else:
            self.step_fn = make_step(network, task, self.optimizer, opt.uncertainty, get_nodata_value(opt.scene),
                                     opt.mindepth, opt.softclamp, opt.hardclamp, opt.inittolerance, world_size, group,
                                     host_reduce)
        self.save_period = 1 if task == 'semantics' else 5
        self.model_path = os.path.join(output_dir, 'model.net')
        self.state = dict(iteration=0, epoch=0, batch=0, steps=0, save_counter=0, epoch_de_facto=0, last_ckpt=0,
                          seed=SAMPLER_SEED)
        # (loss, valid rate) device scalars of the latest steps; e2e: (mean pose loss, summary row of the finishing op)
        self.recent = collections.deque(maxlen=1024)

    def _save_network(self, path):
        if self.rank == 0:
            _atomic_save(state_dict(self.network), path)

    def save_resume(self):
        """model.net + resume.pt, each written whole or not at all.  resume.pt holds everything a bitwise continuation needs,
        the weights included, so it never pairs with a model.net of another step (rank 0 writes; the RNG states are the same
        on every rank: each rank draws the same augmentation parameters)."""
        if self.rank != 0:
            return
        sd = state_dict(self.network)
        _atomic_save(sd, self.model_path)
        _atomic_save(dict(network=sd, optimizer=self.optimizer.state_dict(), scheduler=self.scheduler.state_dict(),
                          state=dict(self.state), rng=_rng_state()), os.path.join(self.output_dir, 'resume.pt'))

    def load_resume(self, path):
        ck = torch.load(path, map_location="cpu", weights_only=False)
        self.network.load_state_dict(ck["network"], strict=True)
        self.optimizer.load_state_dict(ck["optimizer"])
        self.scheduler.load_state_dict(ck["scheduler"])
        self.state.update(ck["state"])
        _set_rng_state(ck["rng"])
        logging.info("Resumed from %s at iteration %d (epoch %d, batch %d)" % (
            path, self.state["iteration"], self.state["epoch"], self.state["batch"]))

    def _batches(self, epoch):
        """(dataset indices, collated batch on the device) of every remaining step of `epoch`."""
        idx = epoch_batches(len(self.dataset), epoch, self.opt.batch_size, self.rank, self.world_size, self.state["seed"])
        idx = idx[self.state["batch"]:] if epoch == self.state["epoch"] else idx
        if self.num_workers > 0:
            loader = torch.utils.data.DataLoader(self.dataset, batch_sampler=idx, num_workers=self.num_workers,
                                                 pin_memory=True, collate_fn=self.dataset.collate_host)
            for b, host in zip(idx, loader):
                yield b, self.dataset.to_gpu(host, self.device, self.network.OUTPUT_SUBSAMPLE)
        else:
            for b in idx:
                yield b, self.dataset.collate_gpu([self.dataset[i] for i in b], self.device, self.network.OUTPUT_SUBSAMPLE)

    def run(self):
        opt, st, n = self.opt, self.state, len(self.dataset)
        max_steps = opt.max_steps if opt.max_steps is not None else math.inf
        log_interval = max(1, opt.log_interval)
        stopped = False
        for epoch in range(st["epoch"], opt.epochs):
            if st["steps"] >= max_steps:
                stopped = True
                break
            logging.info("Optimizer works effectively with a learning rate of {:.6f}".format(
                self.optimizer.param_groups[0]['lr']))
            logging.info("=== Epoch: %d ======================================" % epoch)
            if epoch != st["epoch"]:
                st["epoch"], st["batch"] = epoch, 0
            t0 = time.time()
            for b, (images, gt_poses, gt_labels, focal_lengths, _) in self._batches(epoch):
                # augmentation changes the input size from batch to batch: keep the current size's plans only
                self.network.drop_plans_except(images.shape[0], images.shape[2], images.shape[3])
                if self.e2e:
                    loss, rate = self.step_fn(images, gt_poses, gt_labels, focal_lengths, st["steps"], image0=b[0])
                elif getattr(self.dataset, 'canvas', False):       # every frame has its own scale: all focal lengths
                    loss, rate = self.step_fn(images, gt_poses, gt_labels, focal_lengths.view(-1))
                else:
                    loss, rate = self.step_fn(images, gt_poses, gt_labels, float(focal_lengths.view(-1)[0]))
                self.recent.append((loss, rate))
                st["batch"] += 1
                st["steps"] += 1
                st["iteration"] += len(images) * self.world_size
                if st["steps"] % log_interval == 0:
                    dt = (time.time() - t0) / (log_interval * len(images))
                    if self.e2e:
                        mean_loss, accepted, max_norm, clipped = rate.tolist()
                        logging.info('Iteration: %7d, Epoch: %3d, Pose loss: %.4f, Accepted: %d/%d, Max norm: %.4g, '
                                     'Clipped: %d, Avg Time: %.3fs' % (st["iteration"], epoch, mean_loss, accepted,
                                                                       len(images), max_norm, clipped, dt))
                    else:
                        logging.info('Iteration: %7d, Epoch: %3d, Total loss: %.2f, Valid: %.1f%%, Avg Time: %.3fs' % (
                            st["iteration"], epoch, loss.item(), float(rate) * 100, dt))
                    t0 = time.time()
                snapshot = st["iteration"] > st["save_counter"]                 # train_single_task.py:309-315
                if snapshot:
                    st["save_counter"] = st["iteration"] + n
                    st["epoch_de_facto"] += 1
                    self.scheduler.step()
                if st["iteration"] > st["last_ckpt"] + self.save_period * n or st["last_ckpt"] == 0:     # :317-322
                    st["last_ckpt"] = st["iteration"]
                    self._save_network(os.path.join(self.ckpt_dir, 'ckpt_iter_{:07d}.net'.format(st["iteration"])))
                if snapshot:                                   # after every counter of this step is final
                    logging.info('Saving snapshot of the network to %s.' % self.model_path)
                    self.save_resume()
                if st["steps"] >= max_steps:        # before the next batch is drawn: its augmentation consumes `random`
                    stopped = True
                    break
            else:
                st["epoch"], st["batch"] = epoch + 1, 0
                logging.info('Saving snapshot of the network to %s.' % self.model_path)
                self.save_resume()
                continue
            break
        self.save_resume()
        if not stopped:
            logging.info('Done without errors.')
            if self.rank == 0:
                torch.save(None, os.path.join(self.output_dir, 'FLAG_training_done.nodata'))
                torch.save(None, os.path.join(self.ckpt_dir, 'FLAG_training_done.nodata'))


def common_parser(description, sim_data_chunk_default, task=None):
    """The options shared by train_single_task.py:32-117 and finetune_decoder_single_task.py:29-136 (same names and
    defaults), plus this driver's own: --scene_dir, --output_dir, --max_steps, --log_interval.  `task`: the default of
    --task for an entry point with one task (the option is required otherwise, as in the reference)."""
    import argparse
    p = argparse.ArgumentParser(description=description, formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('scene', help='name of a scene in the dataset folder')
    p.add_argument('--batch_size', type=int, default=4, help='batch size of the dataloader (per rank)')
    p.add_argument('--grayscale', '-grayscale', action='store_true')
    p.add_argument('--real_data_domain', type=str, default='in_place')
    p.add_argument('--real_data_chunk', type=float, default=1.0)
    p.add_argument('--real_only', action='store_true')
    p.add_argument('--sim_data_chunk', type=float, default=sim_data_chunk_default)
    p.add_argument('--task', type=str, required=task is None, default=task)
    p.add_argument('--epoch_plus', '-epoch_plus', action='store_true')
    p.add_argument('--network_in', type=str, default=None)
    p.add_argument('--tiny', '-tiny', action='store_true')
    p.add_argument('--fullsize', '-fullsize', action='store_true')
    p.add_argument('--epochs', '-e', type=int, default=50)
    p.add_argument('--learningrate', '-lr', type=float, default=0.0002)
    p.add_argument('--no_lr_scheduling', action='store_true')
    p.add_argument('--session', '-sid', default='')
    p.add_argument('--ckpt_dir', type=str, default='')
    p.add_argument('--auto_resume', action='store_true')
    p.add_argument('--inittolerance', '-itol', type=float, default=50.0)
    p.add_argument('--mindepth', '-mind', type=float, default=0.1)
    p.add_argument('--softclamp', '-sc', type=float, default=100)
    p.add_argument('--hardclamp', '-hc', type=float, default=1000)
    p.add_argument('--debug', action='store_true')
    p.add_argument('--uncertainty', '-uncertainty', default=None, type=str)
    p.add_argument('--scene_dir', type=str, default=None,
                   help="the scene's dataset folder (default ./datasets/<scene>[-fullsize], as the reference)")
    p.add_argument('--output_dir', type=str, default=None,
                   help="output folder (default ./output/<name derived from the options>, as the reference)")
    p.add_argument('--max_steps', type=int, default=None, help='stop after this many optimiser steps in total')
    p.add_argument('--log_interval', type=int, default=20,
                   help='iterations between log lines (the only points where the step synchronises with the host)')
    p.add_argument('--rotate_poses', action='store_true',
                   help="coord task: draw one rotation per frame and rotate the ground-truth poses with the frames "
                        "(CamLocDataset(rotate_poses=True)); off: one rotation per mini-batch, poses untouched, as the reference")
    p.add_argument('--aug_canvas', action='store_true',
                   help="fixed-size augmentation: one scale and one rotation per frame onto a canvas of the frame's own size "
                        "(CamLocDataset(canvas=True)): the input size never changes, the coord loss reads one focal length per "
                        "frame and the rotated poses; off: one scale and rotation per mini-batch, as the reference")
    return p


def finish_options(opt):
    """The checks that follow parse_args() in both reference parsers."""
    if isinstance(opt.uncertainty, str):
        if opt.uncertainty.lower() == 'none':
            opt.uncertainty = None
        elif opt.uncertainty.lower() == 'mle':
            opt.uncertainty = 'MLE'
    assert opt.uncertainty in [None, 'MLE'], '--uncertainty {} is not supported!'.format(opt.uncertainty)
    assert opt.real_data_domain in ['in_place', 'out_of_place'], \
        '--real_data_domain {:} is not supported!'.format(opt.real_data_domain)
    if opt.rotate_poses and opt.task != 'coord':
        # the other tasks do not read the poses, and the augmentation does not rotate the vectors of a normal map
        raise ValueError('--rotate_poses is for the coord task, not --task {:s}'.format(opt.task))
    return opt


def data_suffix(opt, pairs_name, sim_only_name='-sim_only'):
    """The data part of the reference's output folder names (train_single_task.py:141-165)."""
    s = ''
    if opt.real_data_chunk == 0.0:
        s += sim_only_name + '-sc{:.2f}'.format(opt.sim_data_chunk)
    else:
        s += '-real_only' if opt.real_only else pairs_name
        s += '-ip' if opt.real_data_domain == 'in_place' else '-oop'
        s += '-rc{:.2f}'.format(opt.real_data_chunk)
    return s


def run(opt, basename, encoders_in=None, e2e=False, dataset_options=None):
    """The entry points after option parsing: process group, logging, dataset, network, Trainer.  `e2e`: the Trainer takes
    the end-to-end step; `dataset_options`: keyword arguments of CamLocDataset that replace this function's own."""
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    shared = os.environ.get(SHARED_GPU_ENV, "") not in ("", "0")
    dev = torch.device("cuda", 0 if shared else local_rank)
    torch.cuda.set_device(dev)
    group = None
    if world > 1:
        import torch.distributed as dist
        if shared:
            dist.init_process_group("gloo")              # RCCL refuses two ranks on one device
        else:
            dist.init_process_group("nccl", device_id=dev)
        group = dist.group.WORLD
    try:
        set_random_seed(2021)
        output_dir = os.path.abspath(opt.output_dir or os.path.join('output', basename))
        ckpt_dir = os.path.abspath(os.path.join(opt.ckpt_dir, os.path.basename(output_dir))) if opt.ckpt_dir else output_dir
        resume_path = resume_source(opt, output_dir)
        resume = resume_path is not None
        for d in (output_dir, ckpt_dir):
            os.makedirs(d, exist_ok=True)
        handlers = [logging.StreamHandler()]
        if rank == 0:
            handlers.append(logging.FileHandler(os.path.join(output_dir, 'output.log'), mode='a' if resume else 'w'))
        logging.basicConfig(level=logging.INFO if rank == 0 else logging.WARNING, handlers=handlers, force=True,
                            format='%(asctime)s, %(levelname)s: %(message)s', datefmt="%Y-%m-%d %H:%M:%S")
        logging.getLogger('PIL').setLevel(logging.INFO)
        logging.info('***** %s *****' % ('Automatic resume training' if resume else 'A new training has been started'))
        logging.info('Arg parser: %s' % (opt,))
        logging.info('Path to save data: {:s}; checkpoints: {:s}; ranks: {:d}{:s}'.format(
            output_dir, ckpt_dir, world, ' sharing one GPU' if shared and world > 1 else ''))

        get_nodata_value(opt.scene)
        scene = opt.scene if (opt.task == 'semantics' or not opt.fullsize) else opt.scene + '-fullsize'
        scene_dir = opt.scene_dir or os.path.join('datasets', scene)
        from .dataset import CamLocDataset
        dirs = get_training_dirs(scene_dir, opt.real_data_domain, opt.real_data_chunk, opt.sim_data_chunk, opt.real_only)
        data_kw = dict(coord=opt.task == 'coord', depth=opt.task == 'depth', normal=opt.task == 'normal',
                       semantics=opt.task == 'semantics', augment=True, grayscale=opt.grayscale)
        if opt.rotate_poses:
            data_kw.update(rotate_poses=True)
        if getattr(opt, 'aug_canvas', False):
            data_kw.update(canvas=True)
        data_kw.update(dataset_options or {})
        dataset = CamLocDataset(dirs, **data_kw)
        logging.info("This training uses {:d} frames from {}; {:d} frames per rank and epoch.".format(
            len(dataset), dirs, len(dataset) // world))
        if len(dataset) < world:
            raise ValueError("%d frames cannot be shared by %d ranks" % (len(dataset), world))

        # resuming: the weights come from resume.pt, and encoder checkpoints are not loaded again (learning.py:322)
        network_in = os.path.join(os.path.dirname(resume_path), 'model.net') if resume else opt.network_in
        mean = get_label_mean(opt.scene, opt.task)
        network = config_network(opt.task, opt.tiny, opt.grayscale, opt.uncertainty, opt.fullsize, mean, encoders_in,
                                 getattr(opt, 'reuse_coord_encoder', False), getattr(opt, 'unfreeze_coord_encoder', False),
                                 network_in=network_in)
        network = network.to(dev).train()
        workers = switches.live("XL_TRAIN_WORKERS")
        workers = min(6, (os.cpu_count() or 2) // 2) if workers is None else int(workers)
        trainer = Trainer(network, dataset, opt.task, opt, output_dir, ckpt_dir, dev, rank, world, group,
                          host_reduce=shared, num_workers=workers, e2e=e2e)
        if resume_path:
            trainer.load_resume(resume_path)
        trainer.run()
        return trainer
    finally:
        if world > 1:
            import torch.distributed as dist
            dist.destroy_process_group()
