"""Training of CocoPoseNet on the MI355X path: train_coco_pose_estimation.py.

``Updater`` mirrors the reference's ``Updater.update_core`` (:90-126) on one device: every
iteration runs ``preprocess`` (:76-82, host), then forward + ``compute_loss`` (:41-73) + backward +
``GradientScaling(1/4)`` on conv1_1 .. conv4_4_CPM (:25-38, :213-217) + ``optimizers.Adam`` (:210)
in one call into the HIP library (op_train_step, exact f32).  The schedule is the reference's: the
VGG layers conv1_1 .. conv4_2 start frozen (:219-225) and are enabled at iteration 2000 (:95-100);
alpha 1e-4, then 1e-5 from 100k and 1e-6 from 200k iterations (:102-105).  All of it (Adam's
hyperparameters, the hook's layers and scale, the frozen layers, the re-enable and the alpha at
each schedule edge) is pinned to the reference's own script run under recording stubs
(tests/golden/make_golden_train_host.py -> tests/golden/train/host_schedule.json).

The COCO data pipeline (coco_data_loader.py, pycocotools, getData.sh) needs the dataset and the
network: ``synthetic_batch`` stands in with seeded images and COCO-like maps of random skeletons
(Gaussian heat peaks + unit-vector PAFs on the limbs, the reference's label formulas restated).

``--data poses`` trains from keypoints instead: ``synthetic_poses`` draws integer-valued
(people, 18, 3) poses as parse_coco_annotation makes them, and ``Updater.update_poses`` has the
device generate the targets from them inside the step (labels.py, op_train_step_poses).

``--data samples`` starts one stage earlier, where the reference's loader does: annotated frames of
any size.  ``Updater.update_samples`` draws each sample's augmentation plan on the host (augment.py
``draw_plan``: random resize, rotate, crop, colour, flip, in the reference's draw order), has the
device produce the network-input frames and masks (op_augment) and hands them to ``update_poses``.
``Updater.update_annotated`` starts at the raw COCO annotations: the device makes each image's ignore
mask from the segmentations first (masks.py, op_ignore_masks: gen_ignore_mask.py's ``gen_masks``).

``--dump-samples DIR`` (``--data poses`` or ``samples``) writes the loader's viewer picture of the first
``--dump-count`` training samples (coco_data_loader.py:372-384, ``dump_samples``): the frame beside the
frame with its labels laid over it (overlay.py), without changing the training.

``Validator`` is the reference's (:129-159): every ``--val-interval`` iterations a fixed held-out set
is scored with ``Updater.evaluate`` (op_train_eval: forward + compute_loss only, the training state
is left alone) and ``val/loss``, ``val/paf``, ``val/heat`` join that log entry; at the same points
``Updater.save_snapshot`` writes ``snapshot_iter_N.npz`` (weights, Adam moments, per-layer step
counts, iteration, alpha, frozen layers: extensions.snapshot(), :255) beside ``model_iter_N.npz``, and
``--resume-from FILE`` (the reference's ``--resume FILE``, :265-266) continues from one bit for bit.

    python -m chainer_realtime_multi-person_pose_estimation_amd.train --batchsize 4 --iteration 10
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

from . import _lib
from . import augment as _augment
from . import labels as _labels
from . import masks as _masks
from . import weights as _weights
from .constants import params
from .labels import train_params

VGG_FROZEN = ["conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3", "conv3_4", "conv4_1",
              "conv4_2"]
GRAD_SCALED = VGG_FROZEN + ["conv4_3_CPM", "conv4_4_CPM"]


def preprocess(imgs):
    """train_coco_pose_estimation.py:76-82: (n, h, w, 3) uint8 BGR -> (n, 3, h, w) f32, x/255 - 0.5."""
    x = np.asarray(imgs).astype("f")
    x /= 255
    x -= 0.5
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2))


class GradientScaling(object):
    """train_coco_pose_estimation.py:25-38: multiplies the gradients of ``layer_names`` by ``scale``
    (in f32, ``grad *= scale``) before the optimizer's update.  Registered with
    ``Updater.add_hook`` (the reference's ``optimizer.add_hook``, :213-217); on the device the scale
    is applied inside op_train_step (op_train_set_grad_scale)."""

    name = "GradientScaling"

    def __init__(self, layer_names, scale):
        self.layer_names = layer_names
        self.scale = scale

    def __call__(self, updater):
        for layer_name in self.layer_names:
            updater.ctx.set_grad_scale(updater.names.index(layer_name), self.scale)


def alpha_at(iteration, alpha):
    """update_core's learning-rate schedule (:102-105): the optimizer's alpha before the update of
    ``iteration``, given the alpha in force before it (the reference only ever lowers it)."""
    if 100000 <= iteration < 200000:
        return 1e-5
    if 200000 <= iteration:
        return 1e-6
    return alpha


class Updater(object):
    """One device, one batch shape (n, h, w).  ``update(batch)`` = Updater.update_core (:90-126).

    Set up like the reference's ``__main__`` (:208-225) for ``posenet``: ``optimizers.Adam(alpha=1e-4,
    beta1=0.9, beta2=0.999, eps=1e-8)``, ``GradientScaling(conv1_1 .. conv4_4_CPM, 1/4)`` and, unless
    resuming, conv1_1 .. conv4_2 frozen (re-enabled at iteration 2000).  ``ctx`` (tests) replaces the
    device context: anything with set_weights / set_hyper / enable / set_grad_scale / step / get."""

    def __init__(self, n, h=368, w=368, model=None, device=0, alpha=1e-4, beta1=0.9, beta2=0.999, eps=1e-8,
                 resume=False, ctx=None):
        self.ctx = ctx if ctx is not None else _lib.TrainContext(n, h, w, device)
        self.n = int(n)
        self.insize, self.device = (int(h), int(w)), int(device)
        self.names = [t[0] for t in self.ctx.table]
        self.enabled = {name: True for name in self.names}  # the device's flags, tracked for the snapshot
        self.iteration = 0
        self.alpha, self.beta1, self.beta2, self.eps = alpha, beta1, beta2, eps
        self.hooks = []
        self.ctx.set_weights(model if model is not None else _weights.random_weights(0))
        self.ctx.set_hyper(alpha, beta1, beta2, eps)
        self.add_hook(GradientScaling(GRAD_SCALED, 1 / 4))
        if not resume:
            for name in VGG_FROZEN:
                self.disable_update(name)

    def add_hook(self, hook):
        self.hooks.append(hook)
        hook(self)

    def enable_update(self, name):
        self.ctx.enable(self.names.index(name), True)
        self.enabled[name] = True

    def disable_update(self, name):
        self.ctx.enable(self.names.index(name), False)
        self.enabled[name] = False

    def _schedule(self):
        if self.iteration == 2000:
            for name in VGG_FROZEN:
                self.enable_update(name)
        self.alpha = alpha_at(self.iteration, self.alpha)
        self.ctx.set_hyper(self.alpha, self.beta1, self.beta2, self.eps)

    def update(self, batch):
        """batch = (imgs (n,h,w,3) u8, pafs (n,38,h/8,w/8), heatmaps (n,19,h/8,w/8), ignore_mask (n,h/8,w/8)).
        Returns (loss, paf_loss_log, heatmap_loss_log) as compute_loss does."""
        self._schedule()
        imgs, pafs, heatmaps, ignore_mask = batch
        return self._log(self.ctx.step(preprocess(imgs), pafs, heatmaps, ignore_mask))

    def update_poses(self, imgs, poses_per_frame, mask=None):
        """``update`` from what the reference's loader holds before generate_labels' last three
        lines (coco_data_loader.py:338-340): imgs (n,h,w,3) u8 at the network input size, per frame
        the (people, 18, 3) poses at that size, and the (n,h,w) ignore mask before its dilation
        (None: nothing ignored).  The device makes the targets and runs the iteration."""
        self._schedule()
        return self._log(self.ctx.step_poses(preprocess(imgs), poses_per_frame, mask,
                                             train_params["heatmap_sigma"], train_params["paf_sigma"]))

    def update_samples(self, samples, py_random, np_random):
        """``update`` from what the reference's loader reads: samples = n of (img (h, w, 3) u8 BGR,
        mask (h, w) nonzero = ignored or None, poses (people, 18, 3)) of any sizes.  augment_data
        (coco_data_loader.py:195-205) runs as a host-drawn plan per sample (``py_random`` a
        random.Random, ``np_random`` a np.random.RandomState, consumed in the reference's order) and
        one device call for the pixels, then ``update_poses``."""
        if self.insize[0] != self.insize[1]:
            raise ValueError("update_samples: the crop is square, the context is %d x %d" % self.insize)
        if len(samples) != self.n:
            raise ValueError("update_samples: %d samples, the context holds %d" % (len(samples), self.n))
        imgs, poses, mask = _augment.augment_batch(samples, self.insize[0], py_random, np_random, self.device)
        return self.update_poses(imgs, poses, mask)

    def update_annotated(self, samples, py_random, np_random):
        """``update_samples`` from raw COCO annotations: samples = n of (img (h, w, 3) u8 BGR, all the
        image's annotations as ``COCO.loadAnns`` returns them).  The ignore masks of the batch are made
        on the device (gen_ignore_mask.py's ``gen_masks``; its PNG round trip, ``* 255`` then
        ``== 255``, is lossless), the people are the annotations ``get_img_annotation`` keeps
        (coco_data_loader.py:284-288), parsed by ``parse_coco_annotation``.  A sample without a valid
        person raises ValueError naming its index: the reference's loader draws another image there
        (:351-353), and so does the caller."""
        if len(samples) != self.n:
            raise ValueError("update_annotated: %d samples, the context holds %d" % (len(samples), self.n))
        people = []
        for f, (_, annotations) in enumerate(samples):
            valid = _labels.valid_annotations(annotations)
            if valid is None:
                raise ValueError("update_annotated: sample %d has no valid person annotation" % f)
            people.append(_labels.parse_coco_annotation(valid))
        made = _masks.ignore_masks([(img.shape[0], img.shape[1], annotations) for img, annotations in samples], self.device)
        return self.update_samples([(img, miss, poses) for (img, _), (_, miss), poses in zip(samples, made, people)],
                                   py_random, np_random)

    def _log(self, losses):
        self.iteration += 1
        return self._losses(losses)

    @staticmethod
    def _losses(losses):
        paf_log = [float(v) for v in losses[0::2]]
        heat_log = [float(v) for v in losses[1::2]]
        return sum(paf_log) + sum(heat_log), paf_log, heat_log

    def evaluate(self, batch):
        """``update``'s losses for a batch of m <= n frames without the update (the body of the
        reference's Validator.evaluate loop, :146-157): no schedule step, no backward, no Adam, the
        iteration count stays.  Same return value as ``update``."""
        imgs, pafs, heatmaps, ignore_mask = batch
        return self._losses(self.ctx.eval(preprocess(imgs), pafs, heatmaps, ignore_mask))

    def evaluate_poses(self, imgs, poses_per_frame, mask=None):
        """``evaluate`` with the targets made on the device, arguments as for ``update_poses``."""
        return self._losses(self.ctx.eval_poses(preprocess(imgs), poses_per_frame, mask,
                                                train_params["heatmap_sigma"], train_params["paf_sigma"]))

    def weights(self):
        return self.ctx.get()

    def grads(self):
        return self.ctx.get(grads=True)

    def save_snapshot(self, path):
        """The trainer's state in one npz (no pickle), keys laid out after Chainer's trainer snapshot
        (extensions.snapshot(), :255; modelled on it, not verified against Chainer):
        ``updater/model:main/<layer>/{W,b}``, ``updater/optimizer:main/<layer>/{W,b}/{m,v}``,
        ``updater/optimizer:main/<layer>/t``, ``updater/iteration``, ``updater/alpha`` and
        ``updater/enabled`` (u8 per layer, table order).  ``weights.load_npz`` reads the model out of
        it, so the file also serves as ``--initmodel``."""
        flat = {}
        W, S = self.ctx.get(), self.ctx.get_state()
        for name in self.names:
            flat["updater/model:main/%s/W" % name], flat["updater/model:main/%s/b" % name] = W[name]
            opt = "updater/optimizer:main/%s/" % name
            flat[opt + "W/m"], flat[opt + "W/v"] = S[name]["mW"], S[name]["vW"]
            flat[opt + "b/m"], flat[opt + "b/v"] = S[name]["mb"], S[name]["vb"]
            flat[opt + "t"] = np.int64(S[name]["t"])
        flat["updater/iteration"] = np.int64(self.iteration)
        flat["updater/alpha"] = np.float64(self.alpha)
        flat["updater/enabled"] = np.array([self.enabled[name] for name in self.names], np.uint8)
        with open(path, "wb") as f:  # (np.savez would append .npz to a bare path)
            np.savez(f, **flat)

    def load_snapshot(self, path):
        """``--resume FILE`` (:265-266): weights, then the Adam state (set_weights zeroes it), the
        iteration, alpha and the enabled flags; the hooks are applied again.  The schedule goes on
        as if the run had not stopped."""
        with np.load(path, allow_pickle=False) as z:
            W, S = {}, {}
            for name in self.names:
                W[name] = (z["updater/model:main/%s/W" % name], z["updater/model:main/%s/b" % name])
                opt = "updater/optimizer:main/%s/" % name
                S[name] = dict(mW=z[opt + "W/m"], vW=z[opt + "W/v"], mb=z[opt + "b/m"], vb=z[opt + "b/v"],
                               t=int(z[opt + "t"]))
            iteration, alpha = int(z["updater/iteration"]), float(z["updater/alpha"])
            enabled = np.asarray(z["updater/enabled"])
        if enabled.shape != (len(self.names),):
            raise ValueError("%s: updater/enabled has %s entries, %d layers expected" % (path, enabled.shape,
                                                                                       len(self.names)))
        self.ctx.set_weights(W)
        self.ctx.set_state(S)
        self.iteration = iteration
        self.alpha = alpha
        self.ctx.set_hyper(self.alpha, self.beta1, self.beta2, self.eps)
        for name, on in zip(self.names, enabled):
            (self.enable_update if on else self.disable_update)(name)
        for hook in self.hooks:
            hook(self)


class Validator(object):
    """The reference's Validator (:129-159) over a fixed list of held-out batches: ``evaluate()``
    scores the updater's current weights on each batch (``Updater.evaluate``, or ``evaluate_poses``
    with ``poses=True`` and batches of (imgs, poses_per_frame, mask)) and returns the plain mean over
    batches of the per-batch ``val/loss``, ``val/paf`` and ``val/heat`` (DictSummary.compute_mean: a
    shorter last batch is one observation like any other).  A batch may hold fewer frames than the
    updater's n but not more: it is never split, which would change the mean."""

    def __init__(self, updater, batches, poses=False):
        self.updater = updater
        self.batches = list(batches)
        self.poses = poses

    def evaluate(self):
        if not self.batches:
            raise ValueError("Validator: no batches")
        for batch in self.batches:
            if len(batch[0]) > self.updater.n:
                raise ValueError("Validator: a batch of %d frames, the updater holds %d" % (len(batch[0]),
                                                                                          self.updater.n))
        obs = {"val/loss": [], "val/paf": [], "val/heat": []}
        for batch in self.batches:
            loss, pl, hl = self.updater.evaluate_poses(*batch) if self.poses else self.updater.evaluate(batch)
            obs["val/loss"].append(loss)
            obs["val/paf"].append(sum(pl))
            obs["val/heat"].append(sum(hl))
        return {k: sum(v) / len(v) for k, v in obs.items()}


def synthetic_batch(rng, n, h, w, people=3):
    """Seeded stand-in for CocoDataLoader (coco_data_loader.py:216-268 label formulas): heat maps are
    max-combined Gaussians exp(-d^2 / 2 sigma^2) (sigma 7 px at the input scale) with the background
    channel 1 - max, PAFs the unit limb vector within 8 px of the limb (averaged over people)."""
    h8, w8 = h // 8, w // 8
    imgs = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    heat = np.zeros((n, 19, h8, w8), np.float32)
    paf = np.zeros((n, 38, h8, w8), np.float32)
    yy, xx = np.mgrid[0:h8, 0:w8].astype(np.float32) * 8 + 3.5
    for f in range(n):
        cnt = np.zeros((19, h8, w8), np.float32)
        for _ in range(people):
            c = rng.uniform([0.2 * w, 0.2 * h], [0.8 * w, 0.8 * h])
            joints = c + rng.normal(0, 0.12 * min(h, w), (18, 2))
            for j, (x, y) in enumerate(joints):
                heat[f, j] = np.maximum(heat[f, j], np.exp(-((xx - x) ** 2 + (yy - y) ** 2) / (2 * 7.0 ** 2)))
            for li, (a, b) in enumerate(params["limbs_point"]):
                v = joints[b] - joints[a]
                ln = np.linalg.norm(v)
                if ln < 1e-3:
                    continue
                u = v / ln
                px, py = xx - joints[a][0], yy - joints[a][1]
                along = px * u[0] + py * u[1]
                across = np.abs(px * u[1] - py * u[0])
                m = (along >= 0) & (along <= ln) & (across <= 8.0)
                paf[f, 2 * li][m] += u[0]
                paf[f, 2 * li + 1][m] += u[1]
                cnt[li][m] += 1
        for li in range(19):
            nz = cnt[li] > 0
            paf[f, 2 * li][nz] /= cnt[li][nz]
            paf[f, 2 * li + 1][nz] /= cnt[li][nz]
        heat[f, 18] = 1.0 - heat[f, :18].max(axis=0)
    ignore = (rng.random((n, h8, w8)) < 0.02).astype(np.uint8)
    return imgs, paf, heat, ignore


def synthetic_poses(rng, n, h, w, people=4):
    """Seeded stand-in for parse_coco_annotation + augmentation: per frame a (people, 18, 3) int32
    array, skeletons scattered around a body centre, visibility from {0, 1, 2}."""
    out = []
    for _ in range(n):
        c = rng.uniform([0.2 * w, 0.2 * h], [0.8 * w, 0.8 * h], (people, 1, 2))
        xy = c + rng.normal(0, 0.12 * min(h, w), (people, 18, 2))
        vis = rng.integers(0, 3, (people, 18, 1))
        out.append(np.concatenate([xy, vis], axis=2).astype(np.int32))
    return out


SAMPLE_SIZES = ((240, 320), (333, 500))


def synthetic_samples(rng, n, people=4, sizes=SAMPLE_SIZES):
    """Seeded stand-in for get_img_annotation + parse_coco_annotation: n of (img, mask, poses) at
    mixed sizes, a random image, a sparse ignore mask and ``synthetic_poses`` at that size (every
    person with at least one visible joint, as the loader's min_keypoints filter guarantees)."""
    out = []
    for f in range(n):
        h, w = sizes[f % len(sizes)]
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        mask = rng.random((h, w)) < 0.0005
        poses = synthetic_poses(rng, 1, h, w, people)[0]
        poses[:, 0, 2] = np.maximum(poses[:, 0, 2], 1)
        out.append((img, mask, poses))
    return out


def validation_batches(seed, samples, valbatchsize, insize, data="maps", people=4):
    """The held-out set of the CLI: ``samples`` synthetic frames in batches of ``valbatchsize`` (the
    last one shorter), drawn once from a stream seeded apart from the training stream's."""
    rng = np.random.default_rng([int(seed), 1])
    out = []
    for start in range(0, samples, valbatchsize):
        m = min(valbatchsize, samples - start)
        if data == "poses":
            imgs = rng.integers(0, 256, (m, insize, insize, 3), dtype=np.uint8)
            out.append((imgs, synthetic_poses(rng, m, insize, insize, people),
                        rng.random((m, insize, insize)) < 0.0005))
        else:
            out.append(synthetic_batch(rng, m, insize, insize))
    return out


def dump_samples(out_dir, start, count, imgs, poses, mask, device=0):
    """The reference viewer's picture (coco_data_loader.py:372-384) of up to ``count`` samples of a
    batch as ``update_poses`` takes it, without the window: the labels made on the device
    (labels.make_labels), laid over the frame on the device (overlay.overlay_labels), and
    ``hstack(resized_img, overlay)`` written as sample_<index>.png, index from ``start``.  Returns the
    number written."""
    from . import overlay as _overlay
    from .draw import write_bgr
    k = min(int(count), len(imgs))
    if k < 1:
        return 0
    imgs = [np.ascontiguousarray(a, np.uint8) for a in imgs[:k]]
    h, w = imgs[0].shape[:2]
    pafs, heat, ign = _labels.make_labels(poses[:k], h, w, None if mask is None else np.asarray(mask)[:k], device=device)
    shown = _overlay.overlay_labels(imgs, pafs, heat, ign, device=device)
    os.makedirs(out_dir, exist_ok=True)
    for i in range(k):
        write_bgr(os.path.join(out_dir, "sample_%04d.png" % (start + i)), np.hstack((imgs[i], shown[i])))
    return k


def _mean_entry(observations):
    """LogReport: one entry per interval, every key's mean over the iterations that reported it."""
    keys = []
    for o in observations:
        keys += [k for k in o if k not in keys and k != "iteration"]
    entry = {"iteration": observations[-1]["iteration"]}
    for k in keys:
        vals = [o[k] for o in observations if k in o]
        entry[k] = sum(vals) / len(vals)
    return entry


def main(argv=None, ctx=None):
    ap = argparse.ArgumentParser(description="Train pose estimation (MI355X, synthetic data)")
    ap.add_argument("--arch", "-a", choices=["posenet"], default="posenet")
    ap.add_argument("--batchsize", "-B", type=int, default=10)
    ap.add_argument("--iteration", "-i", type=int, default=10)
    ap.add_argument("--insize", type=int, default=368)
    ap.add_argument("--gpu", "-g", type=int, default=-1, help="HIP device (negative: device 0; no CPU path)")
    ap.add_argument("--initmodel", help="initialise the model from a Chainer npz")
    ap.add_argument("--resume", action="store_true", help="do not freeze the VGG layers")
    ap.add_argument("--out", "-o", default="result/test")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--data", choices=["maps", "poses", "samples"], default="maps",
                    help="maps: host-made synthetic target maps; poses: synthetic keypoints, targets made on the "
                    "device; samples: synthetic annotated frames of mixed sizes, augmented on the device first")
    ap.add_argument("--people", type=int, default=4, help="people per frame (--data poses, samples)")
    ap.add_argument("--resume-from", metavar="FILE", help="continue from a snapshot_iter_N.npz (the reference's "
                    "--resume FILE): weights, Adam state, iteration, alpha and frozen layers")
    ap.add_argument("--valbatchsize", "-b", type=int, default=4, help="validation minibatch size (<= --batchsize)")
    ap.add_argument("--val_samples", type=int, default=100, help="number of validation samples")
    ap.add_argument("--val-interval", type=int, default=1000,
                    help="validate and write snapshot_iter_N.npz + model_iter_N.npz every this many iterations")
    ap.add_argument("--log-interval", type=int, default=1,
                    help="one log entry per this many iterations, holding the means over them")
    ap.add_argument("--test", action="store_true", help="validation interval 10, log interval 1")
    ap.add_argument("--dump-samples", metavar="DIR", help="write hstack(frame, labels laid over it) PNGs of the "
                    "first training samples (--data poses, samples): the reference loader's viewer")
    ap.add_argument("--dump-count", type=int, default=8, help="how many samples --dump-samples writes")
    args = ap.parse_args(argv)
    if args.dump_samples and args.data == "maps":
        ap.error("--dump-samples shows labels made from keypoints: --data poses or samples")
    to_dump = max(args.dump_count, 0) if args.dump_samples else 0  # samples still to be written
    if args.test:
        args.val_interval, args.log_interval = 10, 1
    if args.val_interval < 1 or args.log_interval < 1 or args.valbatchsize < 1 or args.val_samples < 1:
        ap.error("--val-interval, --log-interval, --valbatchsize and --val_samples must be positive")
    model = _weights.load_npz(args.initmodel) if args.initmodel else _weights.random_weights(args.seed)
    up = Updater(args.batchsize, args.insize, args.insize, model=model, device=max(args.gpu, 0), resume=args.resume,
                 ctx=ctx)
    if args.resume_from:
        up.load_snapshot(args.resume_from)
    last = up.iteration + args.iteration
    validator = None
    if last // args.val_interval > up.iteration // args.val_interval:  # a validation point lies ahead
        if args.valbatchsize > args.batchsize:
            ap.error("--valbatchsize must not exceed --batchsize (validation runs in the training context)")
        validator = Validator(up, validation_batches(args.seed, args.val_samples, args.valbatchsize, args.insize,
                                                     "maps" if args.data == "maps" else "poses", args.people),
                              poses=args.data != "maps")
    # (a resumed run draws fresh synthetic batches instead of replaying the stream from its start)
    rng = np.random.default_rng([args.seed, 2, up.iteration] if args.resume_from else args.seed)
    py_random, np_random = random.Random(args.seed), np.random.RandomState(args.seed)  # the augmentation's draws
    os.makedirs(args.out, exist_ok=True)
    log, pending, saved = [], [], None
    for it in range(args.iteration):
        if args.data == "poses":
            imgs = rng.integers(0, 256, (args.batchsize, args.insize, args.insize, 3), dtype=np.uint8)
            poses = synthetic_poses(rng, args.batchsize, args.insize, args.insize, args.people)
            mask = rng.random((args.batchsize, args.insize, args.insize)) < 0.0005
            if to_dump:
                to_dump -= dump_samples(args.dump_samples, args.dump_count - to_dump, to_dump, imgs, poses, mask, up.device)
            t0 = time.perf_counter()
            loss, pl, hl = up.update_poses(imgs, poses, mask)
            dt = time.perf_counter() - t0
            label_ms = up.ctx.last_label_ms()  # device events around the label uploads + kernel
            extra = {"label_ms": label_ms, "step_ms": dt * 1e3 - label_ms}
            note = ", labels %.3f ms, step %.1f ms" % (label_ms, dt * 1e3 - label_ms)
        elif args.data == "samples":
            samples = synthetic_samples(rng, args.batchsize, args.people)
            t0 = time.perf_counter()
            if to_dump:  # update_samples' two steps, with the augmented batch shown in between
                batch = _augment.augment_batch(samples, args.insize, py_random, np_random, up.device)
                augment_ms = _augment.last_ms(up.device)
                to_dump -= dump_samples(args.dump_samples, args.dump_count - to_dump, to_dump, *batch, device=up.device)
                loss, pl, hl = up.update_poses(*batch)
            else:
                loss, pl, hl = up.update_samples(samples, py_random, np_random)
                augment_ms = _augment.last_ms(up.device)
            dt = time.perf_counter() - t0
            label_ms = up.ctx.last_label_ms()
            extra = {"augment_ms": augment_ms, "label_ms": label_ms}
            note = ", augment %.3f ms, labels %.3f ms" % (augment_ms, label_ms)
        else:
            batch = synthetic_batch(rng, args.batchsize, args.insize, args.insize)
            t0 = time.perf_counter()
            loss, pl, hl = up.update(batch)
            dt = time.perf_counter() - t0
            extra, note = {}, ""
        pending.append(dict({"iteration": up.iteration, "main/loss": loss, "main/paf": sum(pl), "main/heat": sum(hl),
                             "elapsed_s": dt}, **extra))
        print("iter %d loss %.6f paf %.6f heat %.6f (%.1f ms%s)" % (up.iteration, loss, sum(pl), sum(hl), dt * 1e3,
                                                                    note), flush=True)
        if up.iteration % args.val_interval == 0:  # Validator, snapshot() and snapshot_object (:252-257)
            val = validator.evaluate()
            pending[-1].update(val)
            print("iter %d val/loss %.6f val/paf %.6f val/heat %.6f" % (up.iteration, val["val/loss"], val["val/paf"],
                                                                       val["val/heat"]), flush=True)
            up.save_snapshot(os.path.join(args.out, "snapshot_iter_%d.npz" % up.iteration))
            _weights.save_npz(os.path.join(args.out, "model_iter_%d.npz" % up.iteration), up.weights())
            saved = up.iteration
        if up.iteration % args.log_interval == 0:
            log.append(pending[0] if args.log_interval == 1 else _mean_entry(pending))
            pending = []
    if pending:  # the iterations after the last full log interval
        log.append(_mean_entry(pending))
    with open(os.path.join(args.out, "log"), "w") as f:
        json.dump(log, f, indent=1)
    if saved != up.iteration:
        _weights.save_npz(os.path.join(args.out, "model_iter_%d.npz" % up.iteration), up.weights())
    return 0


if __name__ == "__main__":
    sys.exit(main())
