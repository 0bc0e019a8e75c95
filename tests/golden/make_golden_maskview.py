"""Generate the MASK-VIEW golden fixtures by running the REFERENCE's own --vis functions.

Run in the build container only (it needs /root/reference, absent on the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_maskview.py

``/root/reference/gen_ignore_mask.py`` is imported UNMODIFIED with the stub modules of
make_golden_labels.py (cv2, pycocotools; ``entity`` is the reference's own), and its
``draw_masks_and_keypoints`` (:48-71) and ``dwaw_gen_masks`` (:39-46) run on a loader made without
``__init__`` whose ``coco`` is a stub: ``annToMask(ann)`` returns the prepared mask of that annotation.
The stub ``cv2`` gets a ``circle`` that records (is the image float64, centre, radius, colour,
thickness) and paints with this package's ``draw.draw_disc``: OpenCV is not installed, so the disc's
pixels stay unpinned against it; everything else (the tint arithmetic, the carried float64 image,
the order of tints and discs, the one cast) is the reference's own code.

Frames are random with rows of 0 and rows of 255.  Cases of draw_masks_and_keypoints (ann_*.npz):
  none                   no annotations (24 x 31)
  crowd / nokp / person  one annotation of each of the three colours (24 x 31), a few keypoints
  twelve                 37 x 53, 12 overlapping annotations of mixed colours whose masks jointly cover
                         most of the frame; keypoints with v in {0, 1, 2}: outside the frame, straddling
                         each border and the corner (0, 0), two overlapping discs of different v inside
                         one annotation, a disc of annotation k under the mask of annotation k + 1
Cases of dwaw_gen_masks (gen_*.npz, 24 x 31): an empty, a partial and a full mask.

Output: tests/golden/maskview/ann_<case>.npz: frame, masks (k, h, w) u8, iscrowd / num_keypoints (k,),
keypoints (k, 51) (x, y, v triples, COCO's 17 per annotation), the recorded calls (call_f64,
call_center, call_radius, call_color, call_thickness) and out; gen_<case>.npz: frame, mask, out
(data only).
"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
draw = importlib.import_module("chainer_realtime_multi-person_pose_estimation_amd.draw")
from make_golden_labels import install_stubs  # noqa: E402

OUT = os.path.join(HERE, "maskview")
CROWD, NOKP, PERSON = (1, 0), (0, 0), (0, 9)  # iscrowd, num_keypoints


class StubCoco(object):
    def __init__(self, masks):
        self.masks = masks

    def annToMask(self, ann):
        return self.masks[ann["k"]].astype(np.uint8)


def frame(rng, h, w):
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    img[2:5] = 0
    img[h // 2:h // 2 + 3] = 255
    img[h - 4, : w // 2] = 255
    img[h - 4, w // 2:] = 0
    return img


def blob(rng, h, w, frac=0.8):
    """A random rectangle-ish blob with ragged edges, covering the centre so that blobs overlap."""
    m = np.zeros((h, w), bool)
    y0, y1 = sorted(rng.integers(0, h, 2))
    x0, x1 = sorted(rng.integers(0, w, 2))
    m[min(y0, h // 2 - 2):max(y1, h // 2 + 2), min(x0, w // 2 - 2):max(x1, w // 2 + 2)] = True
    return m & (rng.random((h, w)) < frac)


def keypoints(triples):
    kp = np.zeros((17, 3), np.int64)
    kp[:len(triples)] = triples
    return kp.ravel()


def cases():
    rng = np.random.default_rng(20250611)
    h, w = 24, 31
    yield "none", frame(rng, h, w), [], [], []
    few = [(5, 6, 1), (20, 12, 2), (0, 0, 0), (29, 22, 1), (12, 12, 2)]
    for name, role in (("crowd", CROWD), ("nokp", NOKP), ("person", PERSON)):
        yield name, frame(rng, h, w), [blob(rng, h, w)], [role], [keypoints(few)]
    h, w = 37, 53
    roles = [PERSON, CROWD, NOKP, PERSON, PERSON, CROWD, NOKP, PERSON, CROWD, PERSON, NOKP, PERSON]
    masks = [blob(rng, h, w, 0.85) for _ in roles]
    masks[0][:, :8] = True   # the borders belong to some mask: jointly most of the frame
    masks[1][:, -8:] = True
    masks[2][:6] = True
    masks[3][-6:] = True
    kps = []
    for k in range(len(roles)):
        t = [(int(rng.integers(0, w)), int(rng.integers(0, h)), int(rng.integers(0, 3))) for _ in range(9)]
        kps.append(t)
    kps[0] += [(-2, 10, 1), (w + 1, 5, 2), (10, -1, 2), (8, h + 2, 1), (0, 0, 2)]     # straddling each border, the corner
    kps[1] += [(-20, -20, 1), (w + 30, 5, 2), (w - 1, h - 1, 1), (3, h + 3, 2)]        # far outside; the far corner; touching
    kps[2] += [(20, 15, 1), (22, 16, 2), (21, 17, 1)]                                # overlapping discs of different v
    ys, xs = np.nonzero(masks[5])                                                    # a disc of annotation 4 under mask 5
    mid = len(ys) // 2
    kps[4] += [(int(xs[mid]), int(ys[mid]), 1), (int(xs[mid // 2]), int(ys[mid // 2]), 2)]
    yield "twelve", frame(rng, h, w), masks, roles, [keypoints(t) for t in kps]


def gen_cases():
    rng = np.random.default_rng(20250612)
    h, w = 24, 31
    yield "empty", frame(rng, h, w), np.zeros((h, w), bool)
    yield "partial", frame(rng, h, w), blob(rng, h, w)
    yield "full", frame(rng, h, w), np.ones((h, w), bool)


def main():
    install_stubs()
    calls = []

    def circle(img, center, radius, color, thickness):
        calls.append((img.dtype == np.float64, (int(center[0]), int(center[1])), int(radius),
                      tuple(int(c) for c in color), int(thickness)))
        assert thickness == -1
        draw.draw_disc(img, center, radius, color)

    sys.modules["cv2"].circle = circle
    mod = importlib.import_module("gen_ignore_mask")
    os.makedirs(OUT, exist_ok=True)
    for name, img, masks, roles, kps in cases():
        h, w = img.shape[:2]
        loader = mod.CocoDataLoader.__new__(mod.CocoDataLoader)
        loader.coco = StubCoco(masks)
        anns = [dict(k=k, iscrowd=r[0], num_keypoints=r[1], keypoints=[int(v) for v in kp])
                for k, (r, kp) in enumerate(zip(roles, kps))]
        del calls[:]
        keep = img.copy()
        out = loader.draw_masks_and_keypoints(img, anns)
        assert np.array_equal(img, keep) and out.dtype == np.uint8 and out.shape == img.shape
        path = os.path.join(OUT, "ann_%s.npz" % name)
        np.savez_compressed(
            path, frame=img, masks=np.array(masks, np.uint8).reshape(len(masks), h, w),
            iscrowd=np.array([r[0] for r in roles], np.int64), num_keypoints=np.array([r[1] for r in roles], np.int64),
            keypoints=np.array(kps, np.int64).reshape(len(kps), 51),
            call_f64=np.array([c[0] for c in calls], bool), call_center=np.array([c[1] for c in calls], np.int64).reshape(-1, 2),
            call_radius=np.array([c[2] for c in calls], np.int64), call_color=np.array([c[3] for c in calls], np.int64).reshape(-1, 3),
            call_thickness=np.array([c[4] for c in calls], np.int64), out=out)
        covered = np.any(masks, axis=0).mean() if len(masks) else 0.0
        print("ann_%-8s %2dx%-2d %2d annotations, %3d circle calls, masks cover %3.0f %%, %d of %d bytes changed, %d bytes" % (
            name, h, w, len(masks), len(calls), 100 * covered, int((out != img).sum()), img.size, os.path.getsize(path)))
    for name, img, mask in gen_cases():
        loader = mod.CocoDataLoader.__new__(mod.CocoDataLoader)
        out = loader.dwaw_gen_masks(img, mask)
        assert out.dtype == np.uint8 and out.shape == img.shape
        path = os.path.join(OUT, "gen_%s.npz" % name)
        np.savez_compressed(path, frame=img, mask=mask, out=out)
        print("gen_%-8s %d of %d bytes changed, %d bytes" % (name, int((out != img).sum()), img.size, os.path.getsize(path)))


if __name__ == "__main__":
    main()
