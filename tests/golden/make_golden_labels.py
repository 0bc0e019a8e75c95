"""Generate the TRAINING-LABEL golden fixtures by running the REFERENCE's own label code.

Run in the build container only (it needs /root/reference, absent on the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_labels.py

``/root/reference/coco_data_loader.py`` is imported with empty stub modules for the absent cv2 /
pycocotools / chainer.dataset (``DatasetMixin`` = object) and for ``models.*`` (which the
reference's own ``entity`` imports for its ``archs`` table); ``entity`` itself is the reference's.
Its UNMODIFIED ``generate_heatmaps``, ``generate_pafs`` (:216-268) and ``parse_coco_annotation``
(:311-332) run on a loader made without ``__init__`` (no COCO object), on an all-zero image of the
case's size (the functions read only its shape), with ``params['heatmap_sigma']`` and
``params['paf_sigma']``.

Cases (every pose seeded and integer-valued, as the reference's int32 pose arrays always are;
visibility drawn from {0, 1, 2}; coordinates up to 10 px outside the frame):
  A  40 x 48, three frames: no people; three people, among them a horizontal limb, a vertical limb
     and a limb whose two joints coincide; 17 people (overlapping limbs, and more records per
     joint and per limb than one LDS chunk of the kernel holds: the counts are printed)
  B  72 x 56, one frame of 5 people
  C  a small synthetic annotation list and its parse_coco_annotation result: one person with both
     shoulders labelled (the Neck is computed), one with a single shoulder

Output: tests/golden/labels/<case>_<frame>.npz (poses, pafs, heatmaps) and parse.npz (data only).
"""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
OUT = os.path.join(HERE, "labels")
MARGIN = 10


def install_stubs():
    for n in ("cv2", "pycocotools", "pycocotools.coco", "chainer", "chainer.dataset", "models", "models.CocoPoseNet",
              "models.FaceNet", "models.HandNet"):
        sys.modules[n] = types.ModuleType(n)
    m = sys.modules
    m["pycocotools.coco"].COCO = object
    m["chainer"].dataset = m["chainer.dataset"]
    m["chainer.dataset"].DatasetMixin = object
    for net in ("CocoPoseNet", "FaceNet", "HandNet"):
        setattr(m["models." + net], net, object)
        setattr(m["models"], net, m["models." + net])
    sys.path.insert(0, REF)


def random_poses(rng, people, h, w):
    poses = np.zeros((people, 18, 3), np.int32)
    poses[:, :, 0] = rng.integers(-MARGIN, w + MARGIN, (people, 18))
    poses[:, :, 1] = rng.integers(-MARGIN, h + MARGIN, (people, 18))
    poses[:, :, 2] = rng.integers(0, 3, (people, 18))
    return poses


def case_frames():
    rng = np.random.default_rng(20240607)
    a1 = random_poses(rng, 3, 40, 48)
    a1[0, 1], a1[0, 8] = (10, 20, 2), (30, 20, 1)    # Neck -> RightWaist: horizontal
    a1[1, 1], a1[1, 11] = (25, 5, 1), (25, 33, 2)    # Neck -> LeftWaist: vertical
    a1[2, 2], a1[2, 3] = (17, 12, 2), (17, 12, 2)    # RightShoulder -> RightElbow: the same point
    yield "a", 40, 48, [np.zeros((0, 18, 3), np.int32), a1, random_poses(rng, 17, 40, 48)]
    yield "b", 72, 56, [random_poses(rng, 5, 72, 56)]


def annotations():
    rng = np.random.default_rng(7)
    anns = []
    for person in range(3):
        kp = np.stack([rng.integers(0, 300, 17), rng.integers(0, 200, 17), rng.integers(0, 3, 17)], axis=1)
        anns.append(kp)
    anns[0][5], anns[0][6] = (101, 50, 2), (60, 81, 1)   # both shoulders: odd sums, truncated midpoint
    anns[1][5], anns[1][6] = (120, 40, 2), (90, 44, 0)   # the left shoulder only
    anns[2][5], anns[2][6] = (0, 0, 0), (0, 0, 0)        # neither
    return [{"keypoints": [int(v) for v in kp.ravel()], "num_keypoints": int((kp[:, 2] > 0).sum()),
             "area": float(40 * 40 + i)} for i, kp in enumerate(anns)]


def main():
    install_stubs()
    loader_mod = importlib.import_module("coco_data_loader")
    entity = importlib.import_module("entity")
    loader = loader_mod.CocoDataLoader.__new__(loader_mod.CocoDataLoader)
    os.makedirs(OUT, exist_ok=True)
    for case, h, w, frames in case_frames():
        img = np.zeros((h, w, 3), np.uint8)
        for i, poses in enumerate(frames):
            heat = loader.generate_heatmaps(img, poses, entity.params["heatmap_sigma"])
            pafs = loader.generate_pafs(img, poses, entity.params["paf_sigma"])
            assert heat.dtype == np.float32 and heat.shape == (19, h, w) and pafs.shape == (38, h, w)
            path = os.path.join(OUT, "%s_%d.npz" % (case, i))
            np.savez_compressed(path, poses=poses, pafs=pafs, heatmaps=heat)
            vis = poses[:, :, 2] > 0
            limbs = np.array([[int(a), int(b)] for a, b in entity.params["limbs_point"]])
            print(path, len(poses), "people", os.path.getsize(path), "bytes; visible per joint", vis.sum(0).tolist(),
                  "per limb", (vis[:, limbs[:, 0]] & vis[:, limbs[:, 1]]).sum(0).tolist())
    anns = annotations()
    poses = loader.parse_coco_annotation(anns)
    np.savez_compressed(os.path.join(OUT, "parse.npz"), keypoints=np.array([a["keypoints"] for a in anns], np.int32),
                        num_keypoints=np.array([a["num_keypoints"] for a in anns], np.int32),
                        area=np.array([a["area"] for a in anns], np.float64), poses=poses)
    print("parse", poses[:, [1, 2, 5]].tolist())


if __name__ == "__main__":
    main()
