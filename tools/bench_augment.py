"""Timing of the augmentation next to the label and step time of the same batch (DESIGN
"Augmentation"): 10 samples of 480 x 640 into 368 x 368, the reference's batch and a COCO-sized frame.

    python tools/bench_augment.py [--rounds 3] [--runs 20] [--steps 5]

op_augment_last_ms (stream events around the uploads and the two kernels) over --rounds rounds of
--runs calls after 3 warm-up calls each; then op_train_last_label_ms and the step's host time (update_poses ends in a device synchronise) over
--steps steps after 2 warm-up steps.  Prints the median, minimum and maximum of every series and one
JSON line.  Needs the device: there is no other path."""
import argparse
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
    print("%-28s median %8.3f ms  min %8.3f  max %8.3f  (n = %d)" % (name, out["median"], out["min"], out["max"], out["n"]))
    return out


def main():
    import importlib
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--insize", type=int, default=368)
    args = ap.parse_args()
    aug = importlib.import_module(PKG + ".augment")
    train = importlib.import_module(PKG + ".train")
    rng = np.random.default_rng(0)
    samples = train.synthetic_samples(rng, args.n, people=4, sizes=((480, 640),))
    py, npr = random.Random(0), np.random.RandomState(0)
    plans, poses = zip(*[aug.draw_plan(p, 480, 640, args.insize, py, npr) for _, _, p in samples])
    imgs, masks = [s[0] for s in samples], [s[1] for s in samples]
    print("plans: resized %s, degrees %s" % ([(p.rw, p.rh) for p in plans], [round(p.degree, 1) for p in plans]))
    result = {"n": args.n, "insize": args.insize, "source": [480, 640]}
    ref = None
    per, wall = [], []
    for rnd in range(args.rounds):
        for _ in range(3):
            out = aug.augment(imgs, masks, plans)
        if ref is None:
            ref = out
        assert np.array_equal(out[0], ref[0]) and np.array_equal(out[1], ref[1])
        ms, ws = [], []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            aug.augment(imgs, masks, plans)
            ws.append((time.perf_counter() - t0) * 1e3)
            ms.append(aug.last_ms(0))
        per += ms
        wall += ws
        series("round %d" % rnd, ms)
    result["augment_ms"] = series("augment (op_augment_last_ms)", per)
    result["augment_host_ms"] = series("  host time of the call", wall)
    lds, fallback = aug.last_paths(0)
    result["pixels_lds"], result["pixels_global"] = lds, fallback
    up = train.Updater(args.n, args.insize, args.insize)
    label, step = [], []
    for it in range(2 + args.steps):
        t0 = time.perf_counter()
        up.update_poses(ref[0], list(poses), ref[1])
        dt = (time.perf_counter() - t0) * 1e3
        if it >= 2:
            label.append(up.ctx.last_label_ms())
            step.append(dt - label[-1])
    up.ctx.close()
    result["label_ms"] = series("labels (op_train_last_label_ms)", label)
    result["step_ms"] = series("step (host time - labels)", step)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
