"""Generate the IGNORE-MASK golden fixtures by running the REFERENCE's own gen_masks.

Run in the build container only (it needs /root/reference, absent on the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_masks.py

``/root/reference/gen_ignore_mask.py`` is imported UNMODIFIED with the stub modules of
make_golden_labels.py (cv2, pycocotools; ``entity`` is the reference's own) and its ``gen_masks``
(:23-37) runs on a loader made without ``__init__`` whose ``coco`` is a stub: ``annToMask(ann)``
returns the prepared random mask of that annotation.  The image is an all-zero array of the case's
size (``gen_masks`` reads only its shape).

Line 30 of the reference subtracts two bool arrays (``mask - intxn``), which current NumPy refuses.
The NumPy of the reference's time computed a bool ``-`` as XOR, and since ``intxn`` is a subset of
``mask`` that equals ``mask & ~intxn``.  So the stub returns an ``ndarray`` subclass whose ``__sub__``
on bools is ``a & ~b``; nothing else of it differs from an ndarray.

Cases (24 x 31 and 17 x 40; masks are random blobs that overlap):
  crowd_first / crowd_last   a crowd before and after a kept person it overlaps (the results differ)
  crowd_crowd                a crowd overlapping an earlier crowd, then a kept person
  thresholds                 num_keypoints 4 / 5 and area 1024 / 1025, the edges of the two tests
  mixed                      seven annotations of every role in a seeded order
  none                       no annotations

Output: tests/golden/masks/gen_<case>.npz: masks (k, h, w) bool, iscrowd / num_keypoints / area (k,),
mask_all, mask_miss (data only).
"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_labels import install_stubs  # noqa: E402

OUT = os.path.join(HERE, "masks")


class OldBool(np.ndarray):
    """bool ``a - b`` as the NumPy of the reference's time gave it for b a subset of a."""

    def __sub__(self, other):
        if self.dtype == bool and np.asarray(other).dtype == bool:
            assert not np.any(np.asarray(other) & ~np.asarray(self)), "the subtrahend is not a subset"
            return (np.asarray(self) & ~np.asarray(other)).view(OldBool)
        return np.ndarray.__sub__(self, other)


class StubCoco(object):
    def __init__(self, masks):
        self.masks = masks

    def annToMask(self, ann):
        return self.masks[ann["k"]].astype(np.uint8).view(OldBool)


def blob(rng, h, w):
    """A random rectangle-ish blob with ragged edges, covering the centre so that blobs overlap."""
    m = np.zeros((h, w), bool)
    y0, y1 = sorted(rng.integers(0, h, 2))
    x0, x1 = sorted(rng.integers(0, w, 2))
    m[min(y0, h // 2 - 2):max(y1, h // 2 + 2), min(x0, w // 2 - 2):max(x1, w // 2 + 2)] = True
    return m & (rng.random((h, w)) < 0.8)


def cases():
    rng = np.random.default_rng(20250316)
    kept, crowd, miss = (0, 9, 5000.0), (1, 0, 5000.0), (0, 2, 5000.0)  # iscrowd, num_keypoints, area
    h, w = 24, 31
    a, b = blob(rng, h, w), blob(rng, h, w)
    yield "crowd_first", h, w, [a, b], [crowd, kept]
    yield "crowd_last", h, w, [b, a], [kept, crowd]
    yield "crowd_crowd", h, w, [blob(rng, h, w) for _ in range(3)], [crowd, crowd, kept]
    yield "thresholds", h, w, [blob(rng, h, w) for _ in range(4)], [(0, 4, 5000.0), (0, 5, 5000.0), (0, 9, 1024.0),
                                                                  (0, 9, 1025.0)]
    h, w = 17, 40
    roles = [kept, miss, crowd, kept, crowd, miss, (0, 5, 1024)]
    yield "mixed", h, w, [blob(rng, h, w) for _ in roles], roles
    yield "none", h, w, [], []


def main():
    install_stubs()
    mod = importlib.import_module("gen_ignore_mask")
    os.makedirs(OUT, exist_ok=True)
    for name, h, w, masks, roles in cases():
        loader = mod.CocoDataLoader.__new__(mod.CocoDataLoader)
        loader.coco = StubCoco(masks)
        anns = [dict(k=k, iscrowd=r[0], num_keypoints=r[1], area=r[2]) for k, r in enumerate(roles)]
        mask_all, mask_miss = loader.gen_masks(np.zeros((h, w, 3), np.uint8), anns)
        mask_all, mask_miss = np.asarray(mask_all), np.asarray(mask_miss)
        assert mask_all.dtype == bool and mask_miss.dtype == bool and mask_all.shape == (h, w)
        path = os.path.join(OUT, "gen_%s.npz" % name)
        np.savez_compressed(path, masks=np.array(masks, bool).reshape(len(masks), h, w),
                            iscrowd=np.array([r[0] for r in roles], np.int64),
                            num_keypoints=np.array([r[1] for r in roles], np.int64),
                            area=np.array([r[2] for r in roles], np.float64), mask_all=mask_all, mask_miss=mask_miss)
        print("%-12s %2dx%-2d %d annotations, all %4d miss %4d pixels, %d bytes" % (
            name, h, w, len(masks), mask_all.sum(), mask_miss.sum(), os.path.getsize(path)))


if __name__ == "__main__":
    main()
