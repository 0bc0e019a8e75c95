"""The --vis viewer of gen_ignore_mask.py, host side (maskview.py): the NumPy statement pinned
to the reference's own draw_masks_and_keypoints / dwaw_gen_masks (tests/golden/maskview/*.npz), the bound
on the carried float64 state, the declared limits and the argument checks of op_annotation_views (they
run before any device call)."""
import ctypes
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN, pkg_module
from test_masks_host import MASKS, ann_of

VIEWS = os.path.join(GOLDEN, "maskview")


@pytest.fixture(scope="module")
def mv():
    return pkg_module("maskview")


def fixture_anns(d):
    """The annotations of an ann_*.npz fixture (the masks come from the fixture, not from a segmentation)."""
    return [dict(id=k + 1, iscrowd=int(c), num_keypoints=int(nk), area=5000.0, keypoints=[int(v) for v in kp])
            for k, (c, nk, kp) in enumerate(zip(d["iscrowd"], d["num_keypoints"], d["keypoints"]))]


def fixture_calls(d):
    return [((int(c[0]), int(c[1])), int(r), tuple(int(v) for v in col), int(t))
            for c, r, col, t in zip(d["call_center"], d["call_radius"], d["call_color"], d["call_thickness"])]


class RecordingRaster(object):
    """Records ``circle`` calls as the fixture's generator does and paints like draw.Raster."""

    def __init__(self):
        self.calls, self.f64 = [], []
        self.paint = pkg_module("draw").Raster()

    def circle(self, img, center, radius, color, thickness):
        self.f64.append(img.dtype == np.float64)
        self.calls.append(((int(center[0]), int(center[1])), int(radius), tuple(int(v) for v in color), int(thickness)))
        self.paint.circle(img, center, radius, color, thickness)


def truncating_variant(mv, frame, anns, masks):
    """The restatement the picture must NOT be: a uint8 image after every annotation."""
    draw = pkg_module("draw")
    img = frame
    for ann, mask in zip(anns, masks):
        img = mv.tint_np(img, mask, mv.ann_color(ann))
        for x, y, v in mv.keypoint_triples(ann):
            if v in mv.DISC_COLORS:
                draw.draw_disc(img, (int(x), int(y)), mv.RADIUS, mv.DISC_COLORS[int(v)])
        img = img.astype(np.uint8)
    return img


# ---- 1. the statement against the reference's own functions ----
def test_fixtures_cover_the_cases():
    names = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(VIEWS, "*.npz")))
    assert names == ["ann_crowd", "ann_nokp", "ann_none", "ann_person", "ann_twelve", "gen_empty", "gen_full", "gen_partial"]
    one = {n: np.load(os.path.join(VIEWS, "ann_%s.npz" % n)) for n in ("crowd", "nokp", "person")}
    assert [(int(d["iscrowd"][0]), int(d["num_keypoints"][0])) for d in one.values()] == [(1, 0), (0, 0), (0, 9)]
    assert len(np.load(os.path.join(VIEWS, "ann_none.npz"))["masks"]) == 0
    gen = {n: np.load(os.path.join(VIEWS, "gen_%s.npz" % n))["mask"] for n in ("empty", "partial", "full")}
    assert not gen["empty"].any() and gen["full"].all() and gen["partial"].any() and not gen["partial"].all()
    for p in glob.glob(os.path.join(VIEWS, "*.npz")):  # frames contain runs of 0 and of 255
        f = np.load(p)["frame"]
        assert (f == 0).all(axis=(1, 2)).any() and (f == 255).all(axis=(1, 2)).any(), p


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(VIEWS, "ann_*.npz"))), ids=os.path.basename)
def test_draw_masks_and_keypoints_np_equals_the_reference(mv, path):
    d = np.load(path)
    rec = RecordingRaster()
    got = mv.draw_masks_and_keypoints_np(d["frame"], fixture_anns(d), masks=d["masks"], raster=rec)
    assert got.dtype == np.uint8 and np.array_equal(got, d["out"])
    assert rec.calls == fixture_calls(d) and rec.f64 == d["call_f64"].tolist()
    # the default raster paints the same discs
    assert np.array_equal(mv.draw_masks_and_keypoints_np(d["frame"], fixture_anns(d), masks=d["masks"]), d["out"])


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(VIEWS, "gen_*.npz"))), ids=os.path.basename)
def test_draw_gen_masks_np_equals_the_reference(mv, path):
    d = np.load(path)
    got = mv.draw_gen_masks_np(d["frame"], d["mask"])
    assert got.dtype == np.uint8 and np.array_equal(got, d["out"])
    if not d["mask"].any():
        assert np.array_equal(got, d["frame"])


def test_no_annotations_return_the_input(mv):
    d = np.load(os.path.join(VIEWS, "ann_none.npz"))
    got = mv.draw_masks_and_keypoints_np(d["frame"], [])
    assert np.array_equal(got, d["frame"]) and np.array_equal(d["out"], d["frame"])


def test_the_twelve_annotation_fixture_is_not_vacuous(mv):
    """What the picture depends on: the unrounded carried state, the order, discs on a float image."""
    d = np.load(os.path.join(VIEWS, "ann_twelve.npz"))
    anns, masks = fixture_anns(d), d["masks"]
    assert len(anns) == 12 and masks.any(axis=0).mean() > 0.9
    assert sorted(set(mv.ann_color(a) for a in anns)) == [(0, 0, 1), (0, 1, 0), (1, 0, 0)]
    trunc = truncating_variant(mv, d["frame"], anns, masks)
    assert int((trunc != d["out"]).sum()) > 100
    rev = mv.draw_masks_and_keypoints_np(d["frame"], anns[::-1], masks=masks[::-1])
    assert int((rev != d["out"]).sum()) > 1000
    assert len(d["call_f64"]) > 40 and d["call_f64"].all()
    h, w = d["frame"].shape[:2]
    c = d["call_center"]
    assert (c[:, 0] < 0).any() and (c[:, 0] >= w).any() and (c[:, 1] < 0).any() and (c[:, 1] >= h).any()
    assert any((x, y) == (0, 0) for x, y in c.tolist())
    # two overlapping discs of different v inside one annotation
    kp = d["keypoints"][2].reshape(-1, 3)
    kp = kp[kp[:, 2] > 0]
    near = [(a, b) for i, a in enumerate(kp) for b in kp[i + 1:] if a[2] != b[2] and abs(a[0] - b[0]) <= 3 and abs(a[1] - b[1]) <= 3]
    assert near
    # a disc of annotation 4 lies under the mask of annotation 5
    assert any(v > 0 and 0 <= x < w and 0 <= y < h and masks[5][y, x] for x, y, v in d["keypoints"][4].reshape(-1, 3))


# ---- 2. the bound on the carried state: what lets the device cast by truncation and skip clear pixels ----
def test_the_carried_state_stays_below_255_5(mv):
    start = np.repeat(np.arange(256, dtype=np.float64).reshape(256, 1, 1), 3, axis=2)
    ones = np.ones((256, 1), np.uint8)
    for colors in (((0, 0, 0),), ((1, 1, 1),), ((1, 0, 0), (0, 1, 0), (0, 0, 1)), ((1, 1, 1), (0, 0, 0))):
        v = start.copy()
        for step in range(64):
            v = mv.tint_np(v, ones, colors[step % len(colors)])
            assert v.dtype == np.float64 and v.min() >= 0.0 and v.max() < 255.5, (colors, step, v.min(), v.max())
            assert not np.signbit(v).any()
    first = mv.tint_np(start.astype(np.uint8), ones, (1, 1, 1))  # the uint8 frame on the first step: the same values
    assert np.array_equal(first, mv.tint_np(start, ones, (1, 1, 1)))


def test_a_clear_mask_leaves_the_state_bitwise_unchanged(mv):
    rng = np.random.default_rng(3)
    v = rng.uniform(0, 255, (40, 50, 3))
    v = mv.tint_np(v, rng.random((40, 50)) < 0.5, (1, 0, 0))  # values as a tint leaves them
    v[0, :5] = 0.0
    v[1, :5] = 255.0
    for color in ((0, 0, 1), (0, 1, 0), (1, 0, 0)):
        got = mv.tint_np(v, np.zeros((40, 50), np.uint8), color)
        assert got.dtype == np.float64 and got.tobytes() == v.tobytes()
    # and a partly clear one changes nothing outside it
    mask = rng.random((40, 50)) < 0.5
    got = mv.tint_np(v, mask, (0, 1, 0))
    assert got[~mask].tobytes() == v[~mask].tobytes() and not np.array_equal(got[mask], v[mask])


# ---- 3. declared limits ----
def with_kp(kp, **kw):
    ann = ann_of([[1, 1, 8, 1, 8, 8]], **kw)
    ann["keypoints"] = kp
    return ann


@pytest.mark.parametrize("ann,word", [
    (with_kp([3, 4, 1, 5], id=4711), "keypoints"),
    (with_kp([3, 4, 1] * 17 + [1], id=4711), "keypoints"),
    (with_kp([3.5, 4, 1], id=4711), "coordinate"),
    (with_kp([3, 32769, 2], id=4711), "coordinate"),
    (with_kp([-32769, 3, 0], id=4711), "coordinate"),
    (with_kp([float("nan"), 3, 1], id=4711), "coordinate"),
    (dict(ann_of(dict(size=[16, 20], counts="0e4f"), id=4711), keypoints=[]), "compressed"),
    (dict(ann_of([[1, 2, 3, 4]], id=4711), keypoints=[]), "polygon"),
])
def test_declared_limits_raise_naming_the_annotation(mv, ann, word):
    img = np.zeros((16, 20, 3), np.uint8)
    for call in (lambda: mv.view_np(img, [ann]), lambda: mv.draw_masks_and_keypoints_np(img, [ann]),
                 lambda: mv.pack_views([(img, [ann])])):
        with pytest.raises(ValueError) as e:
            call()
        assert "4711" in str(e.value) and word in str(e.value)


def test_the_largest_coordinate_and_float_integers_pass(mv):
    img = np.zeros((16, 20, 3), np.uint8)
    mv.view_np(img, [with_kp([32768, -32768, 1, 3.0, 4.0, 2.0])])
    assert mv.keypoint_triples(with_kp([3.0, 4.0, 2.0, 5, 6, 7])).tolist() == [[3, 4, 2], [5, 6, 0]]


@pytest.mark.parametrize("img", [np.zeros((16, 20, 3), np.float64), np.zeros((16, 20), np.uint8), np.zeros((16, 20, 4), np.uint8)])
def test_a_frame_that_is_not_h_w_3_uint8_raises(mv, img):
    for call in (lambda: mv.view_np(img, []), lambda: mv.draw_masks_and_keypoints_np(img, []),
                 lambda: mv.draw_gen_masks_np(img, np.zeros((16, 20), bool)), lambda: mv.pack_views([(img, [])])):
        with pytest.raises(ValueError, match="uint8"):
            call()


# ---- 4. the tiny COCO file through view_np ----
def test_tiny_coco_panels(mv):
    gen = pkg_module("gen_ignore_mask")
    rng = np.random.default_rng(4)
    for img_id, h, w, anns in gen.load_images(os.path.join(MASKS, "tiny_coco.json")):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        panel = mv.panel_np(img, anns)
        assert panel.shape == (h, 2 * w, 3) and panel.dtype == np.uint8
        ann_img, msk_img = mv.view_np(img, anns)
        assert np.array_equal(panel[:, :w], ann_img) and np.array_equal(panel[:, w:], msk_img)
        assert (ann_img != img).any()


# ---- 5. the argument checks of op_annotation_views (before any device call: no device needed) ----
def hand_made():
    rng = np.random.default_rng(5)
    def img(h, w):
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    a1 = dict(ann_of([[1, 1, 8, 1, 8, 8], [2.5, 3, 9, 4, 5, 9.25, 1, 7]], id=1), keypoints=[3, 4, 1, 5, 6, 2, 0, 0, 0])
    a2 = dict(ann_of(dict(size=[10, 12], counts=[7, 20, 93]), id=2, iscrowd=1, num_keypoints=0), keypoints=[])
    a3 = dict(ann_of([[0, 0, 4, 0, 4, 4]], id=3, num_keypoints=0), keypoints=[2, 2, 2])
    return [(img(10, 12), [a1, a2]), (img(6, 5), []), (img(8, 9), [a3])]


def _call(lib, frames, p, n=None, drop=(), null_frame=None):
    def arg(name):
        return None if name in drop or not p[name].size else lib.ptr(p[name])

    n = len(frames) if n is None else n
    outs = [np.zeros(a.shape, np.uint8) for a in frames]
    bgr = (ctypes.c_void_p * len(frames))(*[None if f == null_frame else a.ctypes.data for f, a in enumerate(frames)])
    tab = (ctypes.c_void_p * len(outs))(*[a.ctypes.data for a in outs])
    rc = lib.lib().op_annotation_views(0, n, None if "bgr" in drop else bgr, arg("row_stride"), arg("hw"), arg("ann_offsets"),
                                       arg("ann_role"), arg("ann_tint"), arg("part_offsets"), arg("part_kind"),
                                       arg("data_offsets"), arg("xy"), arg("counts"), arg("kp_offsets"), arg("kp"), tab, tab)
    return rc, lib.last_error()


def test_pack_views(mv):
    frames, p = mv.pack_views(hand_made())
    assert p["kp_offsets"].tolist() == [0, 3, 3, 4] and p["kp_offsets"].dtype == np.int32
    assert p["kp"].tolist() == [[3, 4, 1], [5, 6, 2], [0, 0, 0], [2, 2, 2]] and p["kp"].dtype == np.int32
    assert p["ann_tint"].tolist() == [0, 2, 1] and p["row_stride"].tolist() == [36, 15, 27]
    assert p["ann_offsets"].tolist() == [0, 2, 2, 3] and p["hw"].tolist() == [10, 12, 6, 5, 8, 9]


def test_op_annotation_views_rejects_bad_arguments(mv, lib):
    """Every check runs before the first device call: this passes on a machine without a device."""
    def bad(word, edit=None, **kw):
        frames, p = mv.pack_views(hand_made())
        if edit:
            edit(p)
        rc, msg = _call(lib, frames, p, **kw)
        assert rc == lib.OP_ERR_INVALID and "op_annotation_views" in msg and word in msg, (word, rc, msg)
        assert "op_ignore_masks" not in msg

    def put(name, index, value):
        def edit(p):
            p[name].reshape(-1)[index] = value
        return edit

    bad("n must", n=0)
    bad("n must", n=-3)
    for name in ("bgr", "row_stride", "hw", "ann_offsets", "ann_role", "ann_tint", "part_offsets", "part_kind",
                 "data_offsets", "xy", "counts", "kp_offsets", "kp"):
        bad("null " + name, drop=(name,))
    bad("bgr", null_frame=1)
    for index, value in ((0, 0), (1, 0), (2, -1), (3, 16385), (4, 16385)):
        bad("hw", put("hw", index, value))
    bad("row_stride", put("row_stride", 0, 35))
    bad("row_stride", put("row_stride", 2, 0))
    bad("ann_offsets", put("ann_offsets", 0, 1))
    bad("ann_offsets", put("ann_offsets", 1, 3))
    bad("part_offsets", put("part_offsets", 2, 1))
    bad("data_offsets", put("data_offsets", 0, 2))
    bad("ann_role", put("ann_role", 1, 3))
    bad("part_kind", put("part_kind", 3, 2))
    for value in (np.nan, 65536.5):
        bad("xy", put("xy", 9, value))
    bad("counts", put("counts", 15, 21))
    for value in (3, -1, 7):
        bad("ann_tint", put("ann_tint", 1, value))
    bad("kp_offsets", put("kp_offsets", 0, 1))
    bad("kp_offsets", put("kp_offsets", 2, 2))      # 0 3 2 4: decreases
    for index, value in ((0, 32769), (1, -32769), (9, 40000), (10, -(2 ** 31))):
        bad("kp", put("kp", index, value))
    bad("keypoint 3", put("kp", 10, 32769))          # a later keypoint is checked too, and named
    ms = ctypes.c_double()
    assert lib.lib().op_annotation_views_last_ms(0, None) == lib.OP_ERR_INVALID
    assert lib.lib().op_annotation_views_last_ms(-1, ctypes.byref(ms)) == lib.OP_ERR_INVALID
    assert lib.lib().op_annotation_views_last_ms(64, ctypes.byref(ms)) == lib.OP_ERR_INVALID
