"""The overlay statement (overlay.py) against the reference's own recorded arrays
(tests/golden/overlay/*.npz, made by make_golden_overlay.py) and its own properties.  No device."""
import os
import re

import numpy as np
import pytest

from conftest import REPO, load_golden, pkg_module


@pytest.fixture(scope="module")
def ov():
    return pkg_module("overlay")


def golden(name):
    return load_golden(os.path.join("overlay", name))


@pytest.mark.parametrize("name", ["pafs_0", "pafs_1"])
def test_paf_hsv_is_the_reference_cvtcolor_input(ov, name):
    g = golden(name)
    assert str(g["code"]) == "COLOR_HSV2BGR" and g["blend"].tolist() == [0.6, 0.4, 0.0]
    hsv = ov.paf_hsv_np(ov.mix_pafs_np(g["pafs"]))
    assert hsv.dtype == np.uint8 and np.array_equal(hsv, g["hsv"])
    assert np.array_equal(hsv[..., 1], hsv[..., 2])  # value = saturation


def test_directed_fixture_holds_what_it_is_for(ov):
    g = golden("pafs_0")
    pafs, hsv = g["pafs"], g["hsv"]
    limbs = pafs.reshape(4, 2, 12, 16)
    present = (limbs != 0).any(axis=1)
    assert (present.sum(axis=0) >= 2).any()                 # overlapping limbs
    assert (~present[3] & present[:3].any(axis=0)).any()    # the last limb is zero where earlier ones are not
    mix = ov.mix_pafs_np(pafs)
    assert (np.hypot(mix[0], mix[1]) > 1).any() and hsv[..., 1].max() == 255
    # an average over the limbs present (what overlay_pafs reads as) would be another picture
    count = np.maximum(present.sum(axis=0), 1)
    assert not np.array_equal(ov.paf_hsv_np(mix / count), hsv)
    a = 0.625
    row = [(a, 0), (0, a), (-a, 0.0), (0, -a), (a, a), (-a, a), (-a, -a), (a, -a), (-a, -0.0), (2 * a, 0), (0, 0)]
    hues = [127, 63, 0, 191, 95, 31, 223, 159, 0, 127, 127]
    for y in (0, 11):
        assert [(float(mix[0, y, x]), float(mix[1, y, x])) for x in range(len(row))] == [tuple(map(float, r)) for r in row]
        assert hsv[y, :len(row), 0].tolist() == hues
    assert np.signbit(pafs[1, 11, 8]) and not np.signbit(mix[1, 11, 8])  # -0.0 does not survive the sum onto +0.0


def test_overlay_pafs_is_overlay_paf_of_the_sequential_sum(ov):
    g = golden("pafs_1")
    pafs, img = g["pafs"], g["img"]
    mix = np.zeros((2, 12, 16))
    for l in range(len(pafs) // 2):
        mix = mix + pafs[2 * l:2 * l + 2].astype(np.float64)
    assert np.array_equal(ov.mix_pafs_np(pafs), mix)
    got = ov.overlay_pafs_np(img, pafs)
    assert got.dtype == np.uint8 and np.array_equal(got, ov.overlay_paf_np(img, mix))
    hsv2bgr, blend = pkg_module("augment").hsv2bgr_np, pkg_module("demo").add_weighted
    assert np.array_equal(got, blend(img, 0.6, hsv2bgr(g["hsv"]), 0.4, 0))
    with pytest.raises(ValueError, match="2L"):
        ov.overlay_pafs_np(img, pafs[:3])


def test_jet_index_is_the_reference_applycolormap_input(ov):
    g = golden("heat_0")
    idx = ov.jet_index_np(g["heatmap"])
    assert idx.dtype == np.uint8 and np.array_equal(idx, g["index"])
    assert idx.min() == 0 and idx.max() == 255 and g["blend"].tolist() == [0.6, 0.4, 0.0]
    got = ov.overlay_heatmap_np(g["img"], g["heatmap"])
    assert np.array_equal(got, pkg_module("demo").add_weighted(g["img"], 0.6, ov.jet_lut()[g["index"]], 0.4, 0))
    # network maps overshoot: the clip, and a table of the caller's
    over = np.array([[-0.5, -1e-9, 0.0, 1.0, 1.0 + 1e-6, 7.0]], np.float32)
    assert ov.jet_index_np(over).tolist() == [[0, 0, 0, 255, 255, 255]]
    lut = np.arange(768, dtype=np.uint8).reshape(256, 3)
    img = np.zeros((1, 6, 3), np.uint8)
    assert np.array_equal(ov.overlay_heatmap_np(img, over, lut)[0, 3], np.rint(lut[255] * 0.4))


def test_ignore_mask_is_the_reference_product(ov):
    g = golden("mask_0")
    got = ov.overlay_ignore_mask_np(g["img"], g["mask"])
    assert got.dtype == np.uint8 and np.array_equal(got, g["out"])
    assert (got[g["mask"]] == 0).all() and np.array_equal(got[~g["mask"]], g["img"][~g["mask"]])


def test_jet_lut(ov):
    lut = ov.jet_lut()
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    assert tuple(lut[0]) == (128, 0, 0) and tuple(lut[255]) == (0, 0, 128)
    assert lut is ov.jet_lut() and not lut.flags.writeable
    for ch, peak in ((0, 1), (1, 2), (2, 3)):  # each channel rises to its plateau at v = peak / 4 and falls
        v = lut[:, ch].astype(int)
        top = np.flatnonzero(v == 255)
        assert len(top) and abs(top.mean() / 255 - peak / 4) < 0.01
        assert (np.diff(v[:top[0] + 1]) >= 0).all() and (np.diff(v[top[-1]:]) <= 0).all()
    assert tuple(lut[128])[1] == 255 and abs(int(lut[128, 0]) - 126) <= 1 and abs(int(lut[128, 2]) - 130) <= 1


def test_resize_linear_f32(ov):
    rng = np.random.default_rng(5)
    x = rng.normal(0, 1, (3, 7, 9)).astype(np.float32)
    x[0, 0, 0] = -0.0
    same = ov.resize_linear_f32_np(x, 7, 9)
    assert same is not x and np.array_equal(same.view(np.uint32), x.view(np.uint32))  # bit for bit
    for value in (np.float32(0.1), np.float32(-3.7)):
        c = np.full((2, 6, 6), value, np.float32)
        for oh, ow in ((48, 48), (9, 9), (2, 2), (48, 9)):  # ratios 8, 3/2, 1/3
            out = ov.resize_linear_f32_np(c, oh, ow)
            assert out.shape == (2, oh, ow) and out.dtype == np.float32
            # constant up to rounding: a pass is two rounded products, whose weights sum to 1, and one
            # rounded sum, at most an ulp together; two passes
            assert np.abs(out - value).max() <= 2 * np.spacing(np.abs(value))
    ones = np.ones((1, 6, 6), np.float32)
    assert all((ov.resize_linear_f32_np(ones, s, s) == 1).all() for s in (48, 9, 2))
    # the taps by hand: 2 -> 4 samples at -0.25, 0.25, 0.75, 1.25, clamped to the source
    ramp = np.array([[[0.0, 1.0]]], np.float32)
    assert ov.resize_linear_f32_np(ramp, 1, 4)[0, 0].tolist() == [0.0, 0.25, 0.75, 1.0]
    up = ov.resize_linear_f32_np(x, 56, 72)
    assert up.min() >= x.min() and up.max() <= x.max() and np.array_equal(up[:, 0, 0], x[:, 0, 0])


def test_overlay_np_layers(ov):
    rng = np.random.default_rng(6)
    img = rng.integers(0, 256, (24, 40, 3), dtype=np.uint8)
    keep = img.copy()
    out = ov.overlay_np(img)
    assert out is not img and np.array_equal(out, img)
    pafs = rng.uniform(-0.7, 0.7, (6, 3, 5)).astype(np.float32)
    heat = rng.uniform(0, 1, (4, 3, 5)).astype(np.float32)
    mask = rng.random((3, 5)) < 0.3
    up = lambda m: ov.resize_linear_f32_np(m, 24, 40)
    step = ov.overlay_pafs_np(img, up(pafs))
    assert np.array_equal(ov.overlay_np(img, pafs=pafs), step)
    step = ov.overlay_heatmap_np(step, up(heat).max(axis=0))
    assert np.array_equal(ov.overlay_np(img, pafs, heat), step)
    big = pkg_module("augment").resize_linear_np(mask.astype(np.uint8) * 255, 40, 24) > 0
    want = ov.overlay_ignore_mask_np(step, big)
    assert np.array_equal(ov.overlay_np(img, pafs, heat, mask), want)
    assert np.array_equal(ov.overlay_np(img, pafs, heat, mask.astype(np.uint8)), want)
    assert np.array_equal(ov.overlay_labels_np(img, pafs, heat, mask), ov.overlay_np(img, pafs, heat[:-1], mask))
    assert np.array_equal(img, keep)
    lut = ov.jet_lut()[::-1]
    assert not np.array_equal(ov.overlay_np(img, heatmaps=heat, lut=lut), ov.overlay_np(img, heatmaps=heat))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_maps_raise(ov, bad):
    img = np.zeros((8, 8, 3), np.uint8)
    pafs, heat = np.zeros((2, 4, 4), np.float32), np.zeros((3, 4, 4), np.float32)
    pafs[1, 2, 3] = heat[1, 0, 1] = bad
    with pytest.raises(ValueError, match="pafs.*finite"):
        ov.overlay_np(img, pafs=pafs)
    with pytest.raises(ValueError, match="heatmaps.*finite"):
        ov.overlay_np(img, heatmaps=heat)
    with pytest.raises(ValueError, match="pafs.*finite"):  # refused before the library is asked for
        ov.overlay([img], pafs=[pafs])
    with pytest.raises(ValueError, match="heatmaps.*finite"):
        ov.overlay_labels([img], [np.zeros_like(pafs)], [heat], [None])


def test_hue_margin(ov):
    paf = np.zeros((2, 1, 4))
    paf[:, 0, 0] = (-1.0, 0.0)   # hue 0: exact
    paf[:, 0, 1] = (1.0, 0.0)    # 127.5
    paf[:, 0, 2] = (0.0, 1.0)    # 63.75
    paf[:, 0, 3] = (-1.0, -0.0)  # hue 255: exact
    assert ov.hue_margin(paf) == 0.25
    lvl = 100.0  # a direction on the edge between levels 99 and 100
    ang = (lvl / 255 - 0.5) * -2 * np.pi
    assert ov.hue_margin(np.array([[[np.cos(ang)]], [[np.sin(ang)]]])) < 1e-9


def test_header_declares_the_overlay_exports(lib):
    with open(os.path.join(REPO, "include", "openpose_hip.h")) as f:
        header = f.read()
    for name in ("op_overlay", "op_overlay_staged", "op_overlay_last_ms"):
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in lib.EXPORTED
    assert re.search(r"#define OP_OVERLAY_PAFS 1\b", header) and re.search(r"#define OP_OVERLAY_HEAT 2\b", header)
    ov = pkg_module("overlay")
    assert (ov.OP_OVERLAY_PAFS, ov.OP_OVERLAY_HEAT) == (1, 2)
