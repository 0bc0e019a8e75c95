"""PAFs, heat maps and the ignore mask over frames on the device (op_overlay / op_overlay_staged,
csrc/overlay.hip) against the statement overlay.overlay_np.  Every comparison is full equality with
nothing excluded, under one asserted condition: no pixel's float64 ``hue * 255`` lies within 1e-9 of a
whole number (``assert_hue_margin``).  A device atan2 within the few ulp the OpenCL rules allow a
double-precision atan2 moves ``hue * 255`` by under 1e-12; every other step is an exactly rounded
operation in both worlds.  The seeds were chosen on the CPU so that the statement satisfies it."""
import ctypes
import os
import time

import numpy as np
import pytest

from conftest import load_golden, pkg_module

pytestmark = pytest.mark.gpu

HUE_MARGIN = 1e-9
# (frame h, w), (map h, w): 8x upsample; non-integer ratios and partial tiles; identity; downscale;
# several tiles both ways (and a row stride larger than 3 w)
MIXED = [((40, 56), (5, 7)), ((37, 51), (6, 5)), ((16, 16), (16, 16)), ((9, 13), (20, 30)), ((33, 130), (5, 17))]


@pytest.fixture(scope="module")
def ov():
    return pkg_module("overlay")


def assert_hue_margin(ov, img_hw, pafs):
    if pafs is None:
        return
    mix = ov.mix_pafs_np(ov.resize_linear_f32_np(pafs, *img_hw))
    margin = ov.hue_margin(mix)
    assert margin > HUE_MARGIN, margin


def mixed_batch(seed, paf_ch=38, heat_ch=18):
    rng = np.random.default_rng(seed)
    imgs, pafs, heat, masks = [], [], [], []
    for k, ((h, w), (mh, mw)) in enumerate(MIXED):
        if k == len(MIXED) - 1:  # rows of a wider image: the stride is not 3 w
            imgs.append(rng.integers(0, 256, (h, w + 7, 3), dtype=np.uint8)[:, 2:2 + w])
        else:
            imgs.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        p = rng.normal(0, 0.25, (paf_ch, mh, mw)).astype(np.float32)
        p[:, rng.random((mh, mw)) < 0.3] = 0  # pixels without a limb
        pafs.append(p)
        t = rng.uniform(-0.1, 1.1, (heat_ch, mh, mw)).astype(np.float32)  # overshoots at both ends
        t[:, rng.random((mh, mw)) < 0.3] *= np.float32(0.1)
        heat.append(t)
        masks.append(rng.random((mh, mw)) < 0.25)
    return imgs, pafs, heat, masks


def check(ov, imgs, pafs=None, heat=None, masks=None, lut=None):
    n = len(imgs)
    given = [None if v is None else [None if a is None else a.copy() for a in v] for v in (imgs, pafs, heat, masks)]
    got = ov.overlay(imgs, pafs, heat, masks, lut=lut)
    assert len(got) == n
    for i in range(n):
        p, t, m = (None if v is None else v[i] for v in (pafs, heat, masks))
        assert_hue_margin(ov, imgs[i].shape[:2], p)
        want = ov.overlay_np(imgs[i], p, t, m, lut=lut)
        assert got[i].shape == imgs[i].shape and got[i].dtype == np.uint8
        assert np.array_equal(got[i], want), (i, np.argwhere((got[i] != want).any(axis=2))[:8])
    for v, g in zip((imgs, pafs, heat, masks), given):  # the inputs are unchanged
        if v is not None:
            assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(v, g))
    return got


def test_mixed_batch_in_one_call(ov):
    imgs, pafs, heat, masks = mixed_batch(11)
    assert imgs[-1].strides[0] > imgs[-1].shape[1] * 3
    full = check(ov, imgs, pafs, heat, masks)
    assert all((g != i).any() for g, i in zip(full, imgs))
    # each single layer alone, and none
    only_p = check(ov, imgs, pafs=pafs)
    only_h = check(ov, imgs, heat=heat)
    only_m = check(ov, imgs, masks=masks)
    none = check(ov, imgs)
    for k in range(len(imgs)):
        assert np.array_equal(none[k], imgs[k])
        assert (only_p[k] != only_h[k]).any() and (only_m[k] == 0).any() and (full[k] != only_p[k]).any()
    # layers missing frame by frame, a mask of the frame's own size, and a colour table of the caller's
    pafs2, heat2, masks2 = list(pafs), list(heat), list(masks)
    pafs2[0] = heat2[1] = masks2[2] = pafs2[3] = heat2[3] = masks2[3] = None
    masks2[0] = np.random.default_rng(12).random((40, 56)) < 0.5
    check(ov, imgs, pafs2, heat2, masks2, lut=np.ascontiguousarray(ov.jet_lut()[::-1]))


def test_windows_that_do_not_fit_are_read_in_place(ov):
    """More channels than the workgroup's staged windows hold: the upsampling taps are read from global
    memory, for one layer beside a staged one and for both."""
    rng = np.random.default_rng(13)
    imgs = [rng.integers(0, 256, (40, 56, 3), dtype=np.uint8) for _ in range(3)]
    chans = [(60, 60), (120, 18), (130, 110)]  # 5 x 7 windows: 35 floats per channel, 3584 in all
    pafs = [rng.normal(0, 0.1, (c, 5, 7)).astype(np.float32) for c, _ in chans]
    heat = [rng.uniform(0, 1, (c, 5, 7)).astype(np.float32) ** 8 for _, c in chans]
    check(ov, imgs, pafs, heat)


@pytest.mark.parametrize("name", ["pafs_0", "pafs_1"])
def test_directed_pafs(ov, name):
    """The fixture inputs of the reference's own overlay_pafs, at map size = frame size: the device
    picture is overlay_np's, whose HSV stage is the reference's recorded array."""
    g = load_golden(os.path.join("overlay", name))
    img, pafs = g["img"], g["pafs"]
    assert np.array_equal(ov.paf_hsv_np(ov.mix_pafs_np(pafs)), g["hsv"])
    got = check(ov, [img], pafs=[pafs])[0]
    blend, hsv2bgr = pkg_module("demo").add_weighted, pkg_module("augment").hsv2bgr_np
    assert np.array_equal(got, blend(img, 0.6, hsv2bgr(g["hsv"]), 0.4, 0))


def test_labels_end_to_end(ov):
    L = pkg_module("labels")
    rng = np.random.default_rng(14)
    n, insize = 2, 64
    poses = []
    for i in range(n):
        p = np.zeros((2, 18, 3), np.int32)
        p[:, :, 0] = rng.integers(4, 60, (2, 18))
        p[:, :, 1] = rng.integers(4, 60, (2, 18))
        p[:, :, 2] = rng.integers(0, 3, (2, 18))
        p[:, :2, 2] = 2
        poses.append(p)
    mask = np.zeros((n, insize, insize), bool)
    mask[0, 10:20, 30:50] = mask[1, 40:44, 5:9] = True
    imgs = [rng.integers(0, 256, (insize, insize, 3), dtype=np.uint8) for _ in range(n)]
    pafs, heat, ign = L.make_labels(poses, insize, insize, mask)
    assert pafs.shape == (n, 38, 8, 8) and heat.shape == (n, 19, 8, 8) and ign.any()
    assert ign.sum() > mask.sum() / 64  # dilated
    for i in range(n):
        assert_hue_margin(ov, (insize, insize), pafs[i])
    got = ov.overlay_labels(imgs, pafs, heat, ign)
    for i in range(n):
        want = ov.overlay_labels_np(imgs[i], pafs[i], heat[i], ign[i])
        assert np.array_equal(got[i], want), np.argwhere((got[i] != want).any(axis=2))[:8]
        assert (got[i] != imgs[i]).any() and (want != ov.overlay_np(imgs[i], pafs[i], heat[i], ign[i])).any()


def outcome(c, i):
    try:
        p, s, r = c.fetch_result(i)
        return (0, p.tobytes(), s.tobytes(), r.n_peaks)
    except IndexError:  # the reference's own (pose_detector.py:197) on noise maps
        return ("IndexError",)


def staged_check(ov, c, frames, precise):
    R = pkg_module("render")
    n = len(frames)
    c.synchronize()
    pafs, heat = c.fetch_maps(0, n)
    before = [outcome(c, i) for i in range(n)]
    if precise:
        assert pafs.shape[2:] == frames.shape[1:3]
    else:
        assert pafs.shape[2] < frames.shape[1] and pafs.shape[3] < frames.shape[2]
    for i in range(n):
        assert_hue_margin(ov, frames.shape[1:3], pafs[i])
    for kw in (dict(), dict(heatmaps=False), dict(pafs=False), dict(pafs=False, heatmaps=False)):
        got = ov.overlay_staged(c, 0, n, **kw)
        assert got.shape == frames.shape and got.dtype == np.uint8
        for i in range(n):
            want = ov.overlay_np(frames[i], pafs[i] if kw.get("pafs", True) else None,
                                 heat[i, :18] if kw.get("heatmaps", True) else None)
            assert np.array_equal(got[i], want), (kw, i, np.argwhere((got[i] != want).any(axis=2))[:8])
    one = ov.overlay_staged(c, n - 1, 1)
    assert np.array_equal(one[0], ov.overlay_np(frames[n - 1], pafs[n - 1], heat[n - 1, :18]))
    assert ov.last_ms() > 0
    # frames, maps and results are as they were
    assert np.array_equal(R.render_staged(c, 0, n, [[]] * n), frames)
    pafs2, heat2 = c.fetch_maps(0, n)
    assert np.array_equal(pafs2, pafs) and np.array_equal(heat2, heat)
    assert [outcome(c, i) for i in range(n)] == before


@pytest.mark.parametrize("net", [None, 96])
def test_staged_frames_and_network_maps_in_place(ov, lib, rand_weights, net):
    """net None: the default network input (368 x 488 for these frames), maps about half the frame's
    size, whose tile windows do not fit: read in place.  net 96: the frame's own size, 12 x 16 maps, an
    8x upsample from windows staged out of the network's [row][col][channel] tensor."""
    W = {k: (w, b.copy()) for k, (w, b) in rand_weights.items()}
    for k in ("Mconv7_stage6_L1", "Mconv7_stage6_L2"):  # fewer noise peaks on the random maps
        W[k] = (W[k][0], W[k][1] - np.float32(0.3))
    limits = lib.OpLimits()
    limits.max_batch = 2
    c = lib.Context(0, lib.params_from_dict({"inference_img_size": net}) if net else None, limits)
    try:
        c.set_weights(W)
        frames = np.stack([np.random.default_rng(60 + i).integers(0, 256, (96, 128, 3), dtype=np.uint8) for i in range(2)])
        c.stage_frames(frames)
        with pytest.raises(RuntimeError, match="maps"):  # staged, but no run yet
            ov.overlay_staged(c, 0, 2)
        c.run_staged()
        got = ov.overlay_staged(c, 0, 2)  # queued behind the run
        staged_check(ov, c, frames, precise=False)
        assert np.array_equal(got, ov.overlay_staged(c, 0, 2))
        for bad_first, bad_n in ((-1, 1), (2, 1), (1, 2), (0, 3)):
            with pytest.raises(ValueError, match="staged"):
                ov.overlay_staged(c, bad_first, bad_n)
        if net is None:  # the averaged full-resolution maps: copied through
            c.run_staged_precise()
            staged_check(ov, c, frames, precise=True)
    finally:
        c.close()


def test_staged_overlay_with_nothing_staged(ov, lib):
    c = lib.Context(0)
    try:
        out, lut = np.zeros(16, np.uint8), np.ascontiguousarray(ov.jet_lut())
        rc = lib.lib().op_overlay_staged(c.h, 0, 1, 3, lib.ptr(lut), lib.ptr(out))
        assert rc == lib.OP_ERR_STATE and "staged" in lib.last_error()
        with pytest.raises(RuntimeError, match="staged"):
            ov.overlay_staged(c, 0, 1)
    finally:
        c.close()


def raw_overlay(lib, n=1, hw=(8, 8), stride=None, paf=(2, 4, 4), heat=(1, 4, 4), mask=(4, 4), drop=()):
    """op_overlay with one field set wrong; the arrays are live and large enough for the right call."""
    img = np.zeros((max(hw[0], 1), max(hw[1], 1), 3), np.uint8)
    out = np.zeros_like(img)
    maps = np.zeros(64 * 64, np.float32)
    mk = np.zeros(64 * 64, np.uint8)
    lut = np.zeros((256, 3), np.uint8)
    one = lambda a: (ctypes.c_void_p * 1)(a.ctypes.data)
    i32 = lambda v: np.array(v, np.int32)
    args = dict(bgr=one(img), row_stride=np.array([img.shape[1] * 3 if stride is None else stride], np.int64), hw=i32(hw),
                pafs=one(maps) if paf else None, paf_chw=i32(paf) if paf else None,
                heat=one(maps) if heat else None, heat_chw=i32(heat) if heat else None,
                mask=one(mk) if mask else None, mask_hw=i32(mask) if mask else None, lut=lut, out=one(out))
    for k in drop:  # "name": the array itself is NULL; "name[0]": its entry for frame 0 is
        if k.endswith("[0]"):
            args[k[:-3]] = (ctypes.c_void_p * 1)(None)
        else:
            args[k] = None
    p = lambda v: lib.ptr(v) if isinstance(v, np.ndarray) else v
    rc = lib.lib().op_overlay(0, n, *[p(args[k]) for k in ("bgr", "row_stride", "hw", "pafs", "paf_chw", "heat",
                                                            "heat_chw", "mask", "mask_hw", "lut", "out")])
    return rc, lib.last_error()


@pytest.mark.parametrize("kw, field", [
    (dict(n=0), "n"), (dict(n=-3), "n"),
    (dict(drop=("bgr",)), "bgr"), (dict(drop=("row_stride",)), "row_stride"), (dict(drop=("hw",)), "hw"),
    (dict(drop=("out",)), "out"), (dict(drop=("bgr[0]",)), "bgr"), (dict(drop=("out[0]",)), "out"),
    (dict(drop=("paf_chw",)), "paf_chw"), (dict(drop=("heat_chw",)), "heat_chw"), (dict(drop=("mask_hw",)), "mask_hw"),
    (dict(drop=("lut",)), "lut"),
    (dict(hw=(0, 8)), "hw"), (dict(hw=(8, 16385)), "hw"), (dict(hw=(-1, 8)), "hw"),
    (dict(stride=23), "row_stride"),
    (dict(paf=(3, 4, 4)), "paf_chw"), (dict(paf=(0, 4, 4)), "paf_chw"), (dict(paf=(-2, 4, 4)), "paf_chw"),
    (dict(heat=(0, 4, 4)), "heat_chw"),
    (dict(paf=(2, 0, 4)), "paf_chw"), (dict(paf=(2, 4, 16385)), "paf_chw"),
    (dict(heat=(1, 16385, 4)), "heat_chw"), (dict(heat=(1, 4, 0)), "heat_chw"),
    (dict(mask=(0, 4)), "mask_hw"), (dict(mask=(4, 16385)), "mask_hw"),
])
def test_validation_names_the_field(lib, kw, field):
    rc, msg = raw_overlay(lib, **kw)
    assert rc == lib.OP_ERR_INVALID, (rc, msg)
    assert msg.startswith("op_overlay: ") and field in msg, msg


def test_the_valid_raw_call_passes(lib):
    """The call the validation cases spoil, unspoilt; with NULL entries and without the optional arrays."""
    assert raw_overlay(lib)[0] == lib.OP_OK
    assert raw_overlay(lib, paf=None, heat=None, mask=None, drop=("lut",))[0] == lib.OP_OK
    assert raw_overlay(lib, drop=("pafs[0]", "heat[0]", "mask[0]", "lut"))[0] == lib.OP_OK


def test_non_finite_maps_are_safe_in_the_c_abi(ov, lib):
    """The C ABI does not refuse them (overlay.py does): the call completes, and the pixels whose taps
    reach no such value are the statement's."""
    rng = np.random.default_rng(15)
    img = rng.integers(0, 256, (40, 56, 3), dtype=np.uint8)
    pafs = rng.normal(0, 0.25, (4, 5, 7)).astype(np.float32)
    heat = rng.uniform(0, 1, (3, 5, 7)).astype(np.float32)
    want = ov.overlay_np(img, pafs, heat)
    pafs[1, 0, 0], pafs[2, 0, 1], heat[0, 0, 0], heat[1, 0, 1] = np.nan, np.inf, -np.inf, np.nan
    out = np.zeros_like(img)
    one = lambda a: (ctypes.c_void_p * 1)(a.ctypes.data)
    stride, hw, lut = np.array([56 * 3], np.int64), np.array([40, 56], np.int32), np.ascontiguousarray(ov.jet_lut())
    pd, hd = np.array(pafs.shape, np.int32), np.array(heat.shape, np.int32)  # (named: they outlive the call)
    rc = lib.lib().op_overlay(0, 1, one(img), lib.ptr(stride), lib.ptr(hw), one(pafs), lib.ptr(pd), one(heat),
                              lib.ptr(hd), None, None, lib.ptr(lut), one(out))
    assert rc == lib.OP_OK, lib.last_error()
    assert np.array_equal(out[20:, 24:], want[20:, 24:])  # the taps of these pixels start at sample (2, 2)


def test_timing_of_eight_frames(ov):
    """Prints the device time (op_overlay_last_ms: uploads + kernel) and the host time of overlay_np on
    the same input: 8 frames of 368 x 368 with 46 x 46 maps, 38 + 18 channels, all layers.  No
    threshold: the device time is positive and the pictures are equal."""
    rng = np.random.default_rng(16)
    n, s, m = 8, 368, 46
    imgs = [rng.integers(0, 256, (s, s, 3), dtype=np.uint8) for _ in range(n)]
    pafs = [(rng.normal(0, 0.2, (38, m, m)) * (rng.random((m, m)) < 0.5)).astype(np.float32) for _ in range(n)]
    heat = [(rng.uniform(0, 1, (18, m, m)) ** 6).astype(np.float32) for _ in range(n)]
    masks = [rng.random((m, m)) < 0.05 for _ in range(n)]
    ov.overlay(imgs, pafs, heat, masks)  # first call: module load
    times = []
    for _ in range(5):
        got = ov.overlay(imgs, pafs, heat, masks)
        times.append(ov.last_ms())
    t0 = time.perf_counter()
    want = [ov.overlay_np(*a) for a in zip(imgs, pafs, heat, masks)]
    host_ms = (time.perf_counter() - t0) * 1e3
    for i in range(n):
        assert_hue_margin(ov, (s, s), pafs[i])
        assert np.array_equal(got[i], want[i]), np.argwhere((got[i] != want[i]).any(axis=2))[:8]
    moved = n * (2 * s * s * 3 + 56 * m * m * 4 + m * m) + 768
    print("\nop_overlay_last_ms (8 x 368 x 368, 46 x 46 maps, 38 + 18 channels, mask): median %.3f ms, min %.3f, "
          "max %.3f of 5; overlay_np %.1f ms; %d bytes in and out" % (float(np.median(times)), min(times), max(times),
                                                                     host_ms, moved))
    assert min(times) > 0
