"""Augmentation on the host (augment.py): the plan against the reference's own loader run under a
recording stub cv2 (tests/golden/augment/plan_*.npz), the pixel path's crop, pad and flip against
the reference's own random_crop_img / flip_img (cropflip_*.npz), and the restated OpenCV arithmetic
against its stated properties.  No device is needed: op_augment's argument checks run before any
device call."""
import ctypes
import glob
import os
import random
import re

import numpy as np
import pytest

from conftest import GOLDEN, PKG_NAME, REPO, pkg_module

PLANS = sorted(glob.glob(os.path.join(GOLDEN, "augment", "plan_*.npz")))
CROPFLIPS = sorted(glob.glob(os.path.join(GOLDEN, "augment", "cropflip_*.npz")))


@pytest.fixture(scope="module")
def aug():
    return pkg_module("augment")


def identity_plan(aug, h, w, insize, center, colour=None, flip=False, shift=(0, 0)):
    """Same-size resize, degree 0 (plus a whole-pixel translation), crop centred at ``center``."""
    R = aug.rotation_matrix((w / 2, h / 2), 0.0)
    R[0, 2] += shift[0]
    R[1, 2] += shift[1]
    return aug.AugmentPlan(h=h, w=w, rw=w, rh=h, degree=0.0, R=R, bw=w, bh=h, colour=colour, flip=flip, insize=insize,
                           **aug.crop_window(center, insize, w, h))


def test_fixtures_cover_the_cases():
    assert len(PLANS) >= 12 and len(CROPFLIPS) >= 4
    recs = [np.load(p) for p in PLANS]
    assert {(bool(r["has_colour"]), bool(r["flip"])) for r in recs} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {(int(r["h"]), int(r["w"])) for r in recs} == {(96, 128), (75, 101)}
    assert {int(r["insize"]) for r in recs} == {64, 160}
    pads = []
    for r in recs:
        x_from, y_from, x_to, y_to = r["window"]
        n = int(r["insize"])
        pads.append((x_from > 0, y_from > 0, x_to < n - 1, y_to < n - 1))
    assert any(all(p) for p in pads) and any(not any(p) for p in pads)
    for p in PLANS + CROPFLIPS:
        assert os.path.getsize(p) < 512 * 1024


@pytest.mark.parametrize("path", PLANS, ids=[os.path.basename(p)[:-4] for p in PLANS])
def test_draw_plan_reproduces_the_reference(aug, path):
    r = np.load(path)
    seed, h, w, insize = (int(r[k]) for k in ("seed", "h", "w", "insize"))
    given = r["poses_in"].copy()
    plan, poses = aug.draw_plan(given, h, w, insize, random.Random(seed), np.random.RandomState(seed))
    assert np.array_equal(given, r["poses_in"])  # not mutated (the reference leaves its argument scaled)
    assert (plan.h, plan.w, plan.insize) == (h, w, insize)
    assert (plan.rw, plan.rh) == tuple(r["resize_img"]) == tuple(r["resize_mask"])
    assert (plan.bw, plan.bh) == tuple(r["warp_img_size"]) == tuple(r["warp_mask_size"])
    assert plan.R.dtype == np.float64 and plan.R.tobytes() == r["warp_img_R"].tobytes() == r["warp_mask_R"].tobytes()
    assert (plan.colour is not None) == bool(r["has_colour"])
    if plan.colour is not None:
        assert plan.colour == tuple(r["colour"])
    assert plan.flip == bool(r["flip"])
    assert poses.dtype == np.int32 and np.array_equal(poses, r["poses_out"])
    # the copy window, as the reference's output mask shows it (the stub's rotated mask is all true)
    x_from, y_from, x_to, y_to = r["window"]
    assert (plan.x_from, plan.y_from, plan.x_to, plan.y_to) == (x_from, y_from, x_to, y_to)
    # the reference's caller keeps the resized poses: the truncation of the scaled coordinates
    scaled = r["poses_in"].copy()
    scaled[:, :, :2] = scaled[:, :, :2] * np.array((plan.rw, plan.rh)) / np.array((w, h))
    assert np.array_equal(scaled, r["poses_scaled"])


def test_person_without_a_visible_joint_raises(aug):
    poses = np.load(PLANS[0])["poses_in"].copy()
    poses[-1, :, 2] = 0
    with pytest.raises(ValueError):
        aug.draw_plan(poses, 96, 128, 64, random.Random(0), np.random.RandomState(0))


def test_rotation_matrix_formula(aug):
    import math
    deg, (cx, cy) = 23.75, (50.5, 37.0)
    a, b = math.cos(deg * (math.pi / 180)), math.sin(deg * (math.pi / 180))
    want = np.array([[a, b, (1 - a) * cx - b * cy], [-b, a, b * cx + (1 - a) * cy]])
    assert aug.rotation_matrix((cx, cy), deg).tobytes() == want.tobytes()


@pytest.mark.parametrize("path", CROPFLIPS, ids=[os.path.basename(p)[:-4] for p in CROPFLIPS])
def test_identity_plan_equals_the_reference_crop_and_flip(aug, path):
    """Same-size resize, zero-fraction warp, the 127 pad, the window arithmetic and the flip."""
    r = np.load(path)
    insize = int(r["insize"])
    h, w = r["mask"].shape
    offset = r["poses_in"][0, 0, :2] - r["crop_poses"][0, 0, :2]
    assert insize % 2 == 0
    center = offset + insize // 2 - 1  # offset = int(center - (insize - 1) / 2 + 0.5)
    plan = identity_plan(aug, h, w, insize, center)
    assert plan.offset == tuple(offset)
    img, mask = aug.augment_np(r["img"], r["mask"], plan)
    assert np.array_equal(img, r["crop_img"]) and np.array_equal(mask, r["crop_mask"])
    assert (img == 127).all(axis=2).any() or not any((plan.x_from, plan.y_from, insize - 1 - plan.x_to, insize - 1 - plan.y_to))
    plan.flip = True
    img, mask = aug.augment_np(r["img"], r["mask"], plan)
    assert np.array_equal(img, r["flip_img"]) and np.array_equal(mask, r["flip_mask"])
    poses = aug.flip_poses(r["crop_poses"].copy(), insize)
    assert np.array_equal(poses, r["flip_poses"])


def test_warp_tables(aug):
    """Every set sums to exactly 1 << 15.  A weight of 1.0 does not fit a short
    (saturate_cast<short>(32768) = 32767), so the zero-fraction sets cannot be a single 32768: they
    are 32767 on the pixel itself plus the deficit of 1 on one other tap, and that still reproduces
    every uint8 value whatever the other tap holds."""
    cub, lin = aug.warp_tables()
    assert cub.shape == (1024, 16) and lin.shape == (1024, 4) and cub.dtype == lin.dtype == np.int16
    assert (cub.astype(np.int64).sum(axis=1) == 32768).all() and (lin.astype(np.int64).sum(axis=1) == 32768).all()
    for tab, own in ((cub, 5), (lin, 0)):  # the pixel's own tap: row 1, column 1 of the 4x4; row 0, column 0 of the 2x2
        zero = tab[0].astype(np.int64)
        assert zero[own] == 32767 and sorted(np.delete(zero, own).tolist()) == [0] * (len(zero) - 2) + [1]
    s, other = np.meshgrid(np.arange(256), np.arange(256))
    assert np.array_equal((s * 32767 + other + 16384) >> 15, s)


def test_library_tables_equal_the_numpy_tables(aug):
    """The kernels read the library's host-built tables: the same numbers as augment_np's."""
    cub, lin, sdiv, hdiv = aug.device_tables()
    wc, wl = aug.warp_tables()
    s, h = aug.hsv_tables()
    assert np.array_equal(cub, wc) and np.array_equal(lin, wl) and np.array_equal(sdiv, s) and np.array_equal(hdiv, h)


def test_pure_translation_is_an_exact_shift(aug):
    """Whole-pixel translation: the source shifted, 128 (the warp's border) beyond the source inside
    the rotated image, 127 (the crop's pad) beyond the crop window."""
    rng = np.random.default_rng(5)
    h, w, insize, (tx, ty) = 40, 56, 64, (7, -5)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    img[(img == 127) | (img == 128)] = 3
    mask = rng.random((h, w)) < 0.3
    plan = identity_plan(aug, h, w, insize, (w // 2, h // 2), shift=(tx, ty))
    out, omask = aug.augment_np(img, mask, plan)
    want = np.full((insize, insize, 3), 127, np.uint8)
    wmask = np.zeros((insize, insize), bool)
    rot = np.full((h, w, 3), 128, np.uint8)  # rotated[y, x] = src[y - ty, x - tx]
    rmask = np.zeros((h, w), bool)
    rot[max(ty, 0):h + min(ty, 0), max(tx, 0):w + min(tx, 0)] = img[max(-ty, 0):h - max(ty, 0), max(-tx, 0):w - max(tx, 0)]
    rmask[max(ty, 0):h + min(ty, 0), max(tx, 0):w + min(tx, 0)] = mask[max(-ty, 0):h - max(ty, 0), max(-tx, 0):w - max(tx, 0)]
    want[plan.y_from:plan.y_to + 1, plan.x_from:plan.x_to + 1] = rot[plan.y1:plan.y2 + 1, plan.x1:plan.x2 + 1]
    wmask[plan.y_from:plan.y_to + 1, plan.x_from:plan.x_to + 1] = rmask[plan.y1:plan.y2 + 1, plan.x1:plan.x2 + 1]
    assert np.array_equal(out, want) and np.array_equal(omask, wmask)
    assert (out == 128).all(axis=2).any() and (out == 127).all(axis=2).any()


def test_colour_grey_pixels(aug):
    """s = 0 (and a saturation delta that keeps it 0): b = g = r = clip(v + dv), whatever the hue."""
    grey = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)
    for colour in ((7, -5, 13), (-10, 0, -30), (3, -40, 30)):
        out = aug.distort_colour_np(grey, colour)
        want = np.clip(np.arange(256) + colour[2], 0, 255).astype(np.uint8)
        assert np.array_equal(out, np.repeat(want[None, :, None], 3, axis=2)), colour


def test_colour_pure_hues_survive_a_zero_delta(aug):
    hues = np.array([[[0, 0, 255], [0, 255, 255], [0, 255, 0], [255, 255, 0], [255, 0, 0], [255, 0, 255]]], np.uint8)
    hsv = aug.bgr2hsv_np(hues)
    assert hsv[0, :, 0].tolist() == [0, 30, 60, 90, 120, 150] and (hsv[0, :, 1:] == 255).all()
    assert np.array_equal(aug.distort_colour_np(hues, (0, 0, 0)), hues)


def test_colour_hue_clamps_at_zero(aug):
    """The reference's maximum(minimum(h + d, 255), 0): a hue of 3 lowered by 10 is 0, not 173."""
    px = np.array([[[0, 26, 255]]], np.uint8)  # bgr: h = 3
    hsv = aug.bgr2hsv_np(px)
    assert hsv[0, 0].tolist() == [3, 255, 255]
    clamped = aug.hsv2bgr_np(np.array([[[0, 255, 255]]], np.uint8))
    assert np.array_equal(aug.distort_colour_np(px, (-10, 0, 0)), clamped)
    wrapped = aug.hsv2bgr_np(np.array([[[173, 255, 255]]], np.uint8))
    assert not np.array_equal(clamped, wrapped)
    # and the upper end is not wrapped either: 179 + 10 = 189 goes to HSV2BGR as it is
    top = aug.hsv2bgr_np(np.array([[[179, 200, 200]]], np.uint8))
    assert np.array_equal(aug.hsv2bgr_np(np.array([[[189, 200, 200]]], np.uint8)),
                          aug.distort_colour_np(top, (10, 0, 0))) or aug.bgr2hsv_np(top)[0, 0, 0] != 179


@pytest.mark.parametrize("out_w,out_h", [(113, 84), (226, 170)])
def test_linear_resize_equals_the_oracle(aug, out_w, out_h):
    from oracle.cvresize import resize_linear_u8
    rng = np.random.default_rng(out_w)
    img = rng.integers(0, 256, (75, 101, 3), dtype=np.uint8)
    assert np.array_equal(aug.resize_linear_np(img, out_w, out_h), resize_linear_u8(img, out_w, out_h))
    m = (rng.random((75, 101)) < 0.2).astype(np.uint8)
    assert np.array_equal(aug.resize_linear_np(m, out_w, out_h), resize_linear_u8(m[:, :, None], out_w, out_h)[:, :, 0])
    assert np.array_equal(aug.resize_linear_np(img, 101, 75), img)


def _call(aug, lib, plans, n=None, insize=64, bgr=True, strides=True, use_plans=True, outs=(True, True), imgs=None):
    n = len(plans) if n is None else n
    keep = imgs or [np.zeros((max(p.h, 1), max(p.w, 1), 3), np.uint8) for p in plans]
    ptrs = (ctypes.c_void_p * len(plans))(*[a.ctypes.data if a is not None else None for a in keep])
    st = np.array([a.shape[1] * 3 if a is not None else 0 for a in keep], np.int64)
    cplans = (aug.OpAugmentPlan * len(plans))(*[aug.pack_plan(p) for p in plans])
    out = np.zeros((max(n, 1), insize, insize, 3), np.uint8)
    omask = np.zeros((max(n, 1), insize, insize), np.uint8)
    rc = lib.lib().op_augment(0, n, ptrs if bgr else None, lib.ptr(st) if strides else None, None,
                              cplans if use_plans else None, insize, lib.ptr(out) if outs[0] else None,
                              lib.ptr(omask) if outs[1] else None)
    return rc, lib.last_error()


def test_op_augment_rejects_bad_arguments(aug, lib):
    """Every check runs before the first device call: this passes on a machine without a device."""
    def good():
        return identity_plan(aug, 20, 30, 64, (15, 10), colour=(1, 2, 3))

    def bad(word, **kw):
        rc, msg = _call(aug, lib, **kw)
        assert rc == lib.OP_ERR_INVALID and "op_augment" in msg and word in msg, (word, rc, msg)

    bad("bgr", plans=[good()], bgr=False)
    bad("row_stride", plans=[good()], strides=False)
    bad("plans", plans=[good()], use_plans=False)
    bad("out_bgr", plans=[good()], outs=(False, True))
    bad("out_mask", plans=[good()], outs=(True, False))
    bad("bgr entry", plans=[good()], imgs=[None])
    bad("n must", plans=[good()], n=0)
    bad("insize", plans=[good()], insize=0)
    p = good()
    p.insize = 32
    bad("insize", plans=[p])
    for field, word in (("h", "h, w"), ("w", "h, w"), ("rw", "rw, rh"), ("rh", "rw, rh"), ("bw", "bw, bh"), ("bh", "bw, bh")):
        p = good()
        setattr(p, field, 0)
        bad(word, plans=[p], imgs=[np.zeros((20, 30, 3), np.uint8)])
    for field, word in (("rw", "rw, rh"), ("rh", "rw, rh"), ("bw", "bw, bh"), ("bh", "bw, bh")):
        p = good()
        setattr(p, field, 16385)
        bad(word, plans=[p])
    for bad_value in (np.nan, np.inf):
        p = good()
        p.R[1, 0] = bad_value
        bad("matrix R", plans=[p])
    p = good()
    p.x_to += 1
    bad("window", plans=[p])
    p = good()
    p.x_to, p.x2 = 64, p.x2 + (64 - p.x_to)
    bad("does not fit insize", plans=[p])
    p = good()
    p.y_from, p.y1 = p.y_from - 1, p.y1 - 1
    bad("window", plans=[p])
    p = good()
    p.bw = p.x2  # the window's last column is outside the rotated image
    bad("rotated size", plans=[p])
    for colour, word in (((11, 0, 0), "dh"), ((0, -41, 0), "ds"), ((0, 0, 31), "dv")):
        p = good()
        p.colour = colour
        bad(word, plans=[p])
        with pytest.raises(ValueError):
            p.check()
    # the second plan of a batch is checked too, and named
    p = good()
    p.rw = 0
    rc, msg = _call(aug, lib, plans=[good(), p])
    assert rc == lib.OP_ERR_INVALID and "plan 1" in msg
    ms = ctypes.c_double()
    assert lib.lib().op_augment_last_ms(0, None) == lib.OP_ERR_INVALID
    assert lib.lib().op_augment_last_ms(-1, ctypes.byref(ms)) == lib.OP_ERR_INVALID


def test_plan_struct_mirrors_the_header(aug):
    src = open(os.path.join(REPO, "include", "openpose_hip.h")).read()
    body = re.search(r"typedef struct op_augment_plan \{(.*?)\} op_augment_plan;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r"(int32_t|double)\s+([^;]+);", body):
        for name in names.split(","):
            name = name.strip()
            m = re.fullmatch(r"(\w+)\[(\d+)\]", name)
            fields.append((m.group(1), ctype, int(m.group(2))) if m else (name, ctype, 1))
    got = [(n, "double" if t in (ctypes.c_double, ctypes.c_double * 6) else "int32_t", 6 if t == ctypes.c_double * 6 else 1)
           for n, t in aug.OpAugmentPlan._fields_]
    assert got == fields
    assert ctypes.sizeof(aug.OpAugmentPlan) == 8 * 7 + 4 * 22  # 7 doubles, 22 int32, no padding


def test_header_declares_what_the_binding_lists(lib):
    src = open(os.path.join(REPO, "include", "openpose_hip.h")).read()
    decl = set(re.findall(r"\b(op_[a-z_]+)\s*\(", src))
    assert decl == set(lib.EXPORTED)
    for name in ("op_augment", "op_augment_last_ms", "op_augment_last_paths", "op_augment_tables"):
        assert name in decl and hasattr(lib.lib(), name)


def test_augment_batch_draws_in_sample_order(aug, monkeypatch):
    """augment_batch = draw_plan per sample, in order, from the two generators, then one device
    call: checked here with the device call replaced by augment_np."""
    monkeypatch.setattr(aug, "augment", lambda imgs, masks, plans, device=0: tuple(
        np.stack(v) for v in zip(*[aug.augment_np(i, m, p) for i, m, p in zip(imgs, masks, plans)])))
    rng = np.random.default_rng(9)
    samples = []
    for path in PLANS[:3]:
        r = np.load(path)
        h, w = int(r["h"]), int(r["w"])
        samples.append((rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.random((h, w)) < 0.1, r["poses_in"]))
    imgs, poses, mask = aug.augment_batch(samples, 64, random.Random(4), np.random.RandomState(4))
    assert imgs.shape == (3, 64, 64, 3) and imgs.dtype == np.uint8 and mask.shape == (3, 64, 64) and mask.dtype == bool
    py, npr = random.Random(4), np.random.RandomState(4)
    for f, (img, m, p) in enumerate(samples):
        plan, want = aug.draw_plan(p, img.shape[0], img.shape[1], 64, py, npr)
        assert np.array_equal(poses[f], want)
        wi, wm = aug.augment_np(img, m, plan)
        assert np.array_equal(imgs[f], wi) and np.array_equal(mask[f], wm)
