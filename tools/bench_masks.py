"""Timing of the ignore-mask generation next to the augmentation and the training step
of the same run: 10 images of 480 x 640 with 8 annotations each (7 people as polygons of 20 .. 60
points, roles mixed, and one crowd as an uncompressed RLE).

    python tools/bench_masks.py [--runs 20] [--steps 5]

3 warm-up calls, then --runs calls of masks.ignore_masks: op_ignore_masks_last_ms (stream events
around the uploads and the three kernels) and the host time of the whole call; for scale the host
time of gen_masks_np (the NumPy statement) on the same batch, once; then op_augment_last_ms and the
training step's host time over --steps update_annotated steps after 2 warm-up steps.  Prints the
median, minimum and maximum of every series and one JSON line.  Needs the device: there is no other
path."""
import argparse
import importlib
import json
import os
import random
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PKG = "chainer_realtime_multi-person_pose_estimation_amd"


def series(name, values):
    out = {"median": statistics.median(values), "min": min(values), "max": max(values), "n": len(values)}
    print("%-34s median %9.3f ms  min %9.3f  max %9.3f  (n = %d)" % (name, out["median"], out["min"], out["max"], out["n"]))
    return out


def workload(rng, n, h, w, people=7):
    """n of (h, w, annotations): star-shaped people and one crowd of vertical strips as an RLE."""
    images, next_id = [], 1
    for _ in range(n):
        anns = []
        for k in range(people):
            c = rng.uniform(0.15, 0.85, 2) * [w, h]
            ang = np.sort(rng.uniform(0, 2 * np.pi, int(rng.integers(20, 61))))
            rad = rng.uniform(0.08, 0.25, len(ang)) * min(h, w)
            xy = np.round(c + np.stack([np.cos(ang), np.sin(ang)], axis=1) * rad[:, None], 2)
            kp = np.zeros((17, 3), int)
            kp[:, :2] = np.clip(c + rng.normal(0, 0.05 * min(h, w), (17, 2)), 0, [w - 1, h - 1])
            kp[:, 2] = 2
            few = k % 3 == 2  # a third of the people are below the keypoint threshold: mask_miss
            anns.append(dict(id=next_id, iscrowd=0, num_keypoints=3 if few else 17, area=float(0.05 * h * w),
                             segmentation=[xy.ravel().tolist()], keypoints=kp.ravel().tolist()))
            next_id += 1
        x0 = int(rng.integers(0, w - 80))
        counts = [x0 * h]
        for _ in range(60):
            top, run = int(rng.integers(0, h // 3)), int(rng.integers(h // 4, h // 2))
            counts[-1] += top
            counts += [run, h - top - run]
        counts[-1] += (w - x0 - 60) * h
        anns.insert(int(rng.integers(0, people)), dict(id=next_id, iscrowd=1, num_keypoints=0, area=0.0, keypoints=[0] * 51,
                                                       segmentation=dict(size=[h, w], counts=counts)))
        next_id += 1
        images.append((h, w, anns))
    return images


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--insize", type=int, default=368)
    args = ap.parse_args()
    masks = importlib.import_module(PKG + ".masks")
    aug = importlib.import_module(PKG + ".augment")
    train = importlib.import_module(PKG + ".train")
    rng = np.random.default_rng(0)
    h, w = 480, 640
    images = workload(rng, args.n, h, w)
    result = {"n": args.n, "source": [h, w], "annotations": len(images[0][2])}
    for _ in range(3):
        ref = masks.ignore_masks(images)
    dev, wall = [], []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        out = masks.ignore_masks(images)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(masks.last_ms(0))
    assert all(np.array_equal(a, b) and np.array_equal(c, d) for (a, c), (b, d) in zip(out, ref))
    result["masks_ms"] = series("masks (op_ignore_masks_last_ms)", dev)
    result["masks_host_ms"] = series("  host time of the call", wall)
    t0 = time.perf_counter()
    want = [masks.gen_masks_np(anns, h, w) for _, _, anns in images]
    result["gen_masks_np_ms"] = (time.perf_counter() - t0) * 1e3
    print("%-34s %9.3f ms (once)" % ("gen_masks_np on the host", result["gen_masks_np_ms"]))
    assert all(np.array_equal(a, b) and np.array_equal(c, d) for (a, c), (b, d) in zip(out, want))
    result["miss_pixels"] = int(sum(m.sum() for _, m in out))
    up = train.Updater(args.n, args.insize, args.insize)
    py, npr = random.Random(0), np.random.RandomState(0)
    samples = [(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), anns) for _, _, anns in images]
    mask_ms, augment_ms, label_ms, step = [], [], [], []
    for it in range(2 + args.steps):
        t0 = time.perf_counter()
        up.update_annotated(samples, py, npr)
        dt = (time.perf_counter() - t0) * 1e3
        if it >= 2:
            mask_ms.append(masks.last_ms(0))
            augment_ms.append(aug.last_ms(0))
            label_ms.append(up.ctx.last_label_ms())
            step.append(dt)
    up.ctx.close()
    result["step_masks_ms"] = series("masks inside update_annotated", mask_ms)
    result["augment_ms"] = series("augment (op_augment_last_ms)", augment_ms)
    result["label_ms"] = series("labels (op_train_last_label_ms)", label_ms)
    result["update_annotated_host_ms"] = series("update_annotated (host time)", step)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
