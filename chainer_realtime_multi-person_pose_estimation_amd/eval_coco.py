"""COCO keypoint AP / AR of a model (or of a results file) against a ``person_keypoints_*.json``,
without pycocotools: what ``COCOeval(gt, dt, 'keypoints')`` + ``evaluate / accumulate / summarize``
print, as keypoint_eval.py states it (parity with pycocotools itself is unpinned).

    python -m chainer_realtime_multi-person_pose_estimation_amd.eval_coco \\
        --annotations annotations/person_keypoints_val2017.json --images val2017 \\
        --weights model_iter_N.npz --results results.json

Every image of the annotations file takes part, ids sorted, with or without persons and with or
without detections.  The frames are read with ``draw.read_bgr`` (PIL) from ``--images`` /
``images[*].file_name`` (with ``--device-jpeg`` baseline JPEG files are decoded on the device instead,
the same pixels: jpeg.py) and bucketed by (h, w); each bucket is staged in chunks of at most
``--batch`` frames through ``PoseDetector.run_staged``, and ``keypoint_eval.evaluate_staged``
matches a chunk's poses against its ground truths on the device, where the post-process left them.
The per-image records are accumulated once at the end, on the host.  ``--weights`` takes what
``weights.load_npz`` reads (a Chainer npz, a ``model_iter_N.npz`` or a snapshot of ``train.py``).

    python -m chainer_realtime_multi-person_pose_estimation_amd.eval_coco \\
        --annotations annotations/person_keypoints_val2017.json --results-in results.json

``--results-in`` scores an existing COCO results file with no detector (``keypoint_eval.evaluate``).
The ten summary lines go to stdout; ``--results`` writes the COCO results JSON of the run.
"""
import argparse
import json
import os
import sys

import numpy as np

from . import keypoint_eval as K
from .gen_ignore_mask import load_images


def score_results(images, path, device):
    dets = K.load_results(path)
    none = (np.zeros((0, K.N_KPTS, 3)), np.zeros(0))
    return K.evaluate([dets.get(img_id, none) for img_id, _, _, _, _ in images],
                      [K.gt_tables(anns) for _, _, _, anns, _ in images], device=device)


def run_detector(images, args):
    """-> (the per-image match records in ``images``' order, the COCO results entries)."""
    from . import weights as _weights
    from .draw import read_bgr
    from .pose_detector import PoseDetector
    model = _weights.random_weights(0) if args.random_weights else None
    det = PoseDetector("posenet", weights_file=args.weights, model=model, device=args.gpu, precise=args.precise,
                       max_batch=args.batch)
    ctx = det.staged_context()
    buckets = {}
    for i, (_, h, w, _, _) in enumerate(images):
        buckets.setdefault((h, w), []).append(i)
    records, entries = [None] * len(images), [None] * len(images)
    routes = {"device": 0, "host": 0}
    for (h, w), members in sorted(buckets.items()):
        for start in range(0, len(members), args.batch):
            chunk = members[start:start + args.batch]
            if args.device_jpeg:  # the files go to the device as they are (PoseDetector.run_staged_jpegs)
                n, route = det.run_staged_jpegs([os.path.join(args.images, images[i][4]) for i in chunk], size=(h, w))
                for r in route:
                    routes[r] += 1
            else:
                frames = np.empty((len(chunk), h, w, 3), np.uint8)
                for k, i in enumerate(chunk):
                    img = read_bgr(os.path.join(args.images, images[i][4]))
                    if img.shape != (h, w, 3):
                        raise ValueError("%s is %d x %d, the annotations say %d x %d" % (images[i][4], img.shape[0], img.shape[1], h, w))
                    frames[k] = img
                n = det.run_staged(frames)
            recs = K.evaluate_staged(det, 0, n, [K.gt_tables(images[i][3]) for i in chunk])
            fetched = ctx.fetch_results(0, n) if args.results else [None] * n
            for k, i in enumerate(chunk):
                records[i] = recs[k]
                if args.results:
                    poses, scores, _ = fetched[k]
                    entries[i] = K.results_json(images[i][0], poses, scores)
    if args.device_jpeg:
        print("device-jpeg: %d frames decoded on the device, %d by Pillow on the host" % (routes["device"], routes["host"]),
              file=sys.stderr)
    return records, [e for per_image in entries if per_image for e in per_image]


def main(argv=None):
    ap = argparse.ArgumentParser(description="COCO keypoint AP / AR (OKS) on the device")
    ap.add_argument("--annotations", required=True, help="person_keypoints_{train,val}2017.json")
    ap.add_argument("--images", help="directory of the images (images[*].file_name)")
    ap.add_argument("--weights", help="model file (what weights.load_npz reads)")
    ap.add_argument("--random-weights", action="store_true", help="seeded random weights: a plumbing run")
    ap.add_argument("--precise", action="store_true", help="multi-scale inference (detect_precise)")
    ap.add_argument("--batch", type=int, default=16, help="frames per staged step")
    ap.add_argument("--device-jpeg", action="store_true", help="decode baseline JPEG frames on the device, straight into "
                    "the staged set (PoseDetector.run_staged_jpegs); other files still go through Pillow")
    ap.add_argument("--limit", type=int, default=None, help="only the first K images")
    ap.add_argument("--gpu", type=int, default=0, help="HIP device")
    ap.add_argument("--results", help="write the COCO results JSON of the run here")
    ap.add_argument("--results-in", help="score this COCO results file instead of running a detector")
    args = ap.parse_args(argv)
    if args.batch < 1:
        ap.error("--batch must be positive")
    if args.limit is not None and args.limit < 0:
        ap.error("--limit must not be negative")
    args.gpu = max(args.gpu, 0)
    if args.results_in:
        if args.weights or args.random_weights or args.results or args.device_jpeg:
            ap.error("--results-in runs no detector: no --weights, --random-weights, --results or --device-jpeg")
    else:
        if not args.images:
            ap.error("--images is needed to run the detector")
        if bool(args.weights) == bool(args.random_weights):
            ap.error("one of --weights and --random-weights")
    images = load_images(args.annotations, with_names=True)
    if args.limit is not None:
        images = images[:args.limit]
    if args.results_in:
        result = score_results(images, args.results_in, args.gpu)
    else:
        records, entries = run_detector(images, args)
        result = K.accumulate_np(records)
        result["stats"] = K.summarize(result)
        if args.results:
            with open(args.results, "w") as f:
                json.dump(entries, f)
    for line in K.format_summary(result["stats"]):
        print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
