"""Generate the OVERLAY golden fixtures by running the REFERENCE's own viewer code.

Run in the build container only (it needs /root/reference, absent on the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_overlay.py

``/root/reference/coco_data_loader.py`` is imported with the stub modules of make_golden_labels.py
and a recording stub ``cv2``: ``cvtColor``, ``applyColorMap`` and ``addWeighted`` record their input
arrays and return zeros.  The reference's own, UNMODIFIED ``overlay_pafs`` (:39-50, which calls
``overlay_paf`` :29-37), ``overlay_heatmap`` (:52-55) and ``overlay_ignore_mask`` (:57-59) run on seeded
inputs.  Only data is recorded:

pafs_<k>.npz: ``img`` u8 (12, 16, 3), ``pafs`` f32 (2L, 12, 16), ``hsv`` the uint8 image handed to
``cvtColor``, ``code`` its conversion code's name, ``blend`` the (alpha, beta, gamma) handed to
``addWeighted``.  pafs_0 is directed: overlapping limbs, a last limb that is zero where earlier ones
are not (the ``paf_flags`` quirk: an average would differ), magnitudes above 1, exact axis and
diagonal directions, (-a, +0.0) and (-a, -0.0).  pafs_1 is 5 random limbs.  The seeds are searched
so that ``hue * 255`` of every pixel lies more than 1e-6 from a whole number (hue 0 and 255 apart):
the device's atan2 then lands in the same level as the host's.
heat_0.npz: ``img``, ``heatmap`` f32 (12, 16) in [0, 1] with 0, 1 and values about k / 255, ``index``
the uint8 image handed to ``applyColorMap``, ``blend``.
mask_0.npz: ``img``, ``mask`` bool (12, 16), ``out`` the masked product.

Output: tests/golden/overlay/*.npz (data only).
"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_labels import install_stubs  # noqa: E402

OUT = os.path.join(HERE, "overlay")
H, W = 12, 16
HSV2BGR, JET = 54, 2
calls = []


def install_cv2():
    cv2 = sys.modules["cv2"]
    cv2.COLOR_HSV2BGR, cv2.COLORMAP_JET = HSV2BGR, JET

    def cvt(img, code):
        calls.append(("cvt", img.copy(), code))
        return np.zeros_like(img)

    def colour_map(img, cmap):
        calls.append(("map", img.copy(), cmap))
        return np.zeros(img.shape + (3,), np.uint8)

    def add_weighted(a, alpha, b, beta, gamma):
        calls.append(("blend", a.copy(), b.copy(), (alpha, beta, gamma)))
        return np.zeros_like(a)

    cv2.cvtColor, cv2.applyColorMap, cv2.addWeighted = cvt, colour_map, add_weighted


def margin(pafs):
    mix = np.zeros((2,) + pafs.shape[1:])
    for k in range(0, len(pafs), 2):
        mix += pafs[k:k + 2]
    v = ((np.arctan2(mix[1], mix[0]) / np.pi) / -2 + 0.5) * 255
    d = np.abs(v - np.rint(v))
    d[(v == 0.0) | (v == 255.0)] = 0.5
    return d.min()


def directed(seed):
    rng = np.random.default_rng([seed, 91])
    pafs = np.zeros((8, H, W), np.float32)
    pafs[0:2, 1:9, 1:10] = rng.uniform(-1, 1, (2, 8, 9))     # limb 0 and limb 1 overlap in rows 4..8
    pafs[2:4, 4:11, 5:14] = rng.uniform(-1, 1, (2, 7, 9))
    pafs[4:6, 6:9, 2:8] = rng.uniform(-3, 3, (2, 3, 6))      # magnitudes above 1, over both
    pafs[6:8, 9:11, 11:15] = rng.uniform(-1, 1, (2, 2, 4))   # the last limb: zero where limbs 0 .. 2 are not
    a = np.float32(0.625)
    row = [(a, 0), (0, a), (-a, 0.0), (0, -a), (a, a), (-a, a), (-a, -a), (a, -a), (-a, -0.0), (2 * a, 0), (0, 0)]
    pafs[:, 11, :] = 0
    pafs[:, 0, :] = 0
    for x, (u, v) in enumerate(row):  # exact directions: row 11 through limb 0, row 0 split over limbs 1 and 3
        pafs[0, 11, x], pafs[1, 11, x] = u, v
        pafs[2, 0, x], pafs[7, 0, x] = u, v
    return pafs


def main():
    install_stubs()
    install_cv2()
    mod = importlib.import_module("coco_data_loader")
    loader = mod.CocoDataLoader.__new__(mod.CocoDataLoader)
    os.makedirs(OUT, exist_ok=True)
    names = {HSV2BGR: "COLOR_HSV2BGR", JET: "COLORMAP_JET"}

    def random_pafs(seed):
        return np.random.default_rng([seed, 92]).uniform(-0.6, 0.6, (10, H, W)).astype(np.float32)

    for k, make in enumerate((directed, random_pafs)):
        seed = next(s for s in range(1000) if margin(make(s)) > 1e-6)
        pafs = make(seed)
        img = np.random.default_rng([seed, 93]).integers(0, 256, (H, W, 3), dtype=np.uint8)
        given = pafs.copy()
        del calls[:]
        loader.overlay_pafs(img, pafs)
        assert [c[0] for c in calls] == ["cvt", "blend"] and np.array_equal(pafs, given)
        (_, hsv, code), (_, a, b, blend) = calls
        assert hsv.dtype == np.uint8 and hsv.shape == (H, W, 3) and np.array_equal(a, img)
        path = os.path.join(OUT, "pafs_%d.npz" % k)
        np.savez_compressed(path, seed=seed, img=img, pafs=pafs, hsv=hsv, code=names[code], blend=np.array(blend, np.float64))
        print(path, "seed", seed, "margin %.3g" % margin(pafs), "hue levels", len(np.unique(hsv[..., 0])),
              os.path.getsize(path), "bytes")

    rng = np.random.default_rng([0, 94])
    heat = rng.uniform(0, 1, (H, W)).astype(np.float32)
    heat[0, :4] = [0.0, 1.0, 0.5, 1e-6]
    ks = np.arange(1, W + 1, dtype=np.float32) * np.float32(15)
    heat[1], heat[2] = ks / np.float32(255), np.nextafter(ks / np.float32(255), np.float32(0))
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    del calls[:]
    loader.overlay_heatmap(img, heat)
    assert [c[0] for c in calls] == ["map", "blend"]
    (_, index, cmap), (_, a, b, blend) = calls
    assert index.dtype == np.uint8 and index.shape == (H, W) and names[cmap] == "COLORMAP_JET"
    path = os.path.join(OUT, "heat_0.npz")
    np.savez_compressed(path, img=img, heatmap=heat, index=index, blend=np.array(blend, np.float64))
    print(path, "indices", int(index.min()), "..", int(index.max()), os.path.getsize(path), "bytes")

    mask = rng.random((H, W)) < 0.3
    del calls[:]
    out = loader.overlay_ignore_mask(img, mask)
    assert not calls and out.dtype == np.uint8 and out.shape == img.shape
    path = os.path.join(OUT, "mask_0.npz")
    np.savez_compressed(path, img=img, mask=mask, out=out)
    print(path, "masked", int(mask.sum()), "of", mask.size, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
