"""Generate the AUGMENTATION golden fixtures by running the REFERENCE's own loader code.

Run in the build container only (it needs /root/reference, absent on the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_augment.py

``/root/reference/coco_data_loader.py`` is imported with the stub modules of make_golden_labels.py
and a recording stub ``cv2``: ``resize`` and ``warpAffine`` return zero arrays of the requested size (the mask's ``warpAffine`` an
array of ones, so that the output mask shows the crop's copy window),
``getRotationMatrix2D`` is the formula (angle * (pi / 180), scale 1, float64), ``cvtColor(BGR2HSV)``
returns a constant 100 so that the input of the ``HSV2BGR`` call reveals the three drawn deltas, and
``flip`` is ``[:, ::-1]``.  Only data is recorded.

plan_<k>.npz: ``random.seed(s); np.random.seed(s)`` and one UNMODIFIED ``augment_data`` (:195-205) on
a zero image, over sources of 96x128 and 75x101 and insize 64 and 160: the input poses, both resize
sizes, both warpAffine matrices (float64) and sizes, the deltas or none, flipped or not, the output
poses, and that the caller's array was left scaled.  The seeds are searched so that colour and flip
each occur with and without the other, one crop is padded on every side and one on none; the
coverage table is printed.

cropflip_<k>.npz: the reference's own ``random_crop_img`` (:126-160) then ``flip_img`` (:175-193,
with the stub flip) on a random uint8 image and a random mask: inputs, seed, outputs and poses.

Output: tests/golden/augment/*.npz (data only).
"""
import importlib
import math
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_labels import install_stubs  # noqa: E402

OUT = os.path.join(HERE, "augment")
BGR2HSV, HSV2BGR = 40, 54
calls = []


def install_cv2():
    cv2 = sys.modules["cv2"]
    cv2.INTER_CUBIC, cv2.BORDER_CONSTANT, cv2.COLOR_BGR2HSV, cv2.COLOR_HSV2BGR, cv2.MORPH_DILATE = 2, 0, BGR2HSV, HSV2BGR, 1

    def resize(img, shape, **kw):
        calls.append(("resize", img.shape, tuple(shape), kw))
        return np.zeros((shape[1], shape[0]) + img.shape[2:], img.dtype)

    def rotation(center, degree, scale):
        rad = degree * (math.pi / 180)
        a, b = math.cos(rad) * scale, math.sin(rad) * scale
        return np.array([[a, b, (1 - a) * center[0] - b * center[1]], [-b, a, b * center[0] + (1 - a) * center[1]]])

    def warp(img, R, dsize, **kw):
        calls.append(("warp", img.shape, np.array(R, np.float64), tuple(dsize), kw))
        return (np.ones if img.ndim == 2 else np.zeros)((dsize[1], dsize[0]) + img.shape[2:], img.dtype)

    def cvt(img, code):
        calls.append(("cvt", code, img[0, 0].copy()))
        return np.full(img.shape, 100, np.uint8) if code == BGR2HSV else img

    def flip(img, code):
        assert code == 1
        calls.append(("flip",))
        return img[:, ::-1]

    cv2.resize, cv2.getRotationMatrix2D, cv2.warpAffine, cv2.cvtColor, cv2.flip = resize, rotation, warp, cvt, flip


def case_poses(seed, h, w):
    rng = np.random.default_rng([seed, 77])
    people = 1 + seed % 3
    poses = np.zeros((people, 18, 3), np.int32)
    c = rng.integers([w // 4, h // 4], [3 * w // 4, 3 * h // 4], (people, 1, 2))
    spread = min(h, w) // (2 if (seed // 4) % 2 else 5)  # wide skeletons are scaled down, narrow ones up
    poses[:, :, :2] = c + rng.integers(-spread, spread, (people, 18, 2))
    poses[:, :, 2] = rng.integers(0, 3, (people, 18))
    poses[:, 0, 2], poses[:, 1, 2] = 2, 1
    return poses


def run_plan(loader, seed, h, w, insize):
    loader.insize = insize
    poses = case_poses(seed, h, w)
    given = poses.copy()
    random.seed(seed)
    np.random.seed(seed)
    del calls[:]
    img, mask, out = loader.augment_data(np.zeros((h, w, 3), np.uint8), np.zeros((h, w), bool), poses)
    names = [c[0] for c in calls]
    assert names[:4] == ["resize", "resize", "warp", "warp"] and out.dtype == np.int32 and out is not poses
    assert img.shape == (insize, insize, 3) and img.dtype == np.uint8 and mask.shape == (insize, insize)
    r0, r1, w0, w1 = calls[:4]
    assert w0[4] == dict(flags=2, borderMode=0, borderValue=127.5) and w1[4] == {} and r0[3] == {} and r1[3] == {}
    cvts = [c for c in calls if c[0] == "cvt"]
    colour = None
    if cvts:
        assert [c[1] for c in cvts] == [BGR2HSV, HSV2BGR]
        colour = cvts[1][2].astype(np.int32) - 100
    shown = mask[:, ::-1] if names.count("flip") == 2 else mask  # True where the crop copied from the rotated image
    ys, xs = np.nonzero(shown)
    window = np.array([xs.min(), ys.min(), xs.max(), ys.max()] if len(xs) else [0, 0, -1, -1], np.int32)
    assert shown.sum() == (window[2] - window[0] + 1) * (window[3] - window[1] + 1)
    rec = dict(seed=seed, window=window, h=h, w=w, insize=insize, poses_in=given, poses_scaled=poses, resize_img=np.array(r0[2]),
               resize_mask=np.array(r1[2]), warp_img_R=w0[2], warp_mask_R=w1[2], warp_img_size=np.array(w0[3]),
               warp_mask_size=np.array(w1[3]), has_colour=colour is not None,
               colour=colour if colour is not None else np.zeros(3, np.int32), flip=names.count("flip") == 2,
               poses_out=out)
    assert names.count("flip") in (0, 2)
    return rec


def main():
    install_stubs()
    install_cv2()
    mod = importlib.import_module("coco_data_loader")
    loader = mod.CocoDataLoader.__new__(mod.CocoDataLoader)
    os.makedirs(OUT, exist_ok=True)

    # candidates in a fixed order; a greedy pass keeps the seeds that add coverage, then fills up to 12
    sizes = [(96, 128, 64), (75, 101, 160), (96, 128, 160), (75, 101, 64)]
    cands = [run_plan(loader, seed, *sizes[seed % 4]) for seed in range(200)]

    def features(rec):
        f = {"colour" if rec["has_colour"] else "plain", "flip" if rec["flip"] else "straight",
             ("colour" if rec["has_colour"] else "plain") + "+" + ("flip" if rec["flip"] else "straight"),
             "%dx%d->%d" % (rec["h"], rec["w"], rec["insize"])}
        pads = pad_sides(rec)
        if all(pads):
            f.add("padded on every side")
        if not any(pads):
            f.add("padded on no side")
        return f

    def pad_sides(rec):
        x_from, y_from, x_to, y_to = rec["window"]
        return x_from > 0, y_from > 0, x_to < rec["insize"] - 1, y_to < rec["insize"] - 1

    keep, seen = [], set()
    for rec in cands:
        f = features(rec)
        if not f <= seen:
            keep.append(rec)
            seen |= f
    for rec in cands:
        if len(keep) >= 12:
            break
        if not any(rec is k for k in keep):
            keep.append(rec)
    keep.sort(key=lambda r: r["seed"])
    print("seed  source   insize  resized   degree   rotated  colour          flip   padded (l, t, r, b)")
    for k, rec in enumerate(keep):
        path = os.path.join(OUT, "plan_%d.npz" % k)
        np.savez_compressed(path, **rec)
        R = rec["warp_img_R"]
        print("%4d  %3dx%-3d  %5d  %4dx%-4d %7.2f  %4dx%-4d %-15s %-5s  %s  %d bytes" % (
            rec["seed"], rec["h"], rec["w"], rec["insize"], rec["resize_img"][1], rec["resize_img"][0],
            math.degrees(math.atan2(R[0, 1], R[0, 0])), rec["warp_img_size"][1], rec["warp_img_size"][0],
            rec["colour"].tolist() if rec["has_colour"] else "-", rec["flip"],
            "".join("x" if v else "." for v in pad_sides(rec)), os.path.getsize(path)))

    for k, (h, w, insize, seed) in enumerate([(75, 101, 64, 3), (96, 128, 160, 4), (75, 101, 160, 5), (96, 128, 64, 6)]):
        loader.insize = insize
        rng = np.random.default_rng([seed, 78])
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        mask = rng.random((h, w)) < 0.3
        poses = case_poses(seed, h, w)
        given = poses.copy()
        random.seed(seed)
        np.random.seed(seed)
        cimg, cmask, cposes = loader.random_crop_img(img, mask, poses)
        crop_poses = cposes.copy()
        fimg, fmask, fposes = loader.flip_img(cimg, cmask, cposes)
        assert cimg.dtype == np.uint8 and cmask.dtype == bool and fmask.dtype == bool
        path = os.path.join(OUT, "cropflip_%d.npz" % k)
        np.savez_compressed(path, seed=seed, insize=insize, img=img, mask=mask, poses_in=given, crop_img=cimg,
                            crop_mask=cmask, crop_poses=crop_poses, flip_img=np.ascontiguousarray(fimg),
                            flip_mask=np.ascontiguousarray(fmask), flip_poses=fposes)
        off = given[0, 0, :2] - crop_poses[0, 0, :2]
        print(path, "offset", off.tolist(), "pad values", sorted(set(np.unique(cimg[..., 0]).tolist()) & {127}),
              os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
