"""Ignore masks from COCO segmentations, host side (masks.py): the NumPy statement
(gen_masks pinned to the reference's own function, the polygon rasteriser held from two sides),
pack_annotations and the argument checks of op_ignore_masks (they run before any device call)."""
import ctypes
import glob
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, pkg_module

MASKS = os.path.join(GOLDEN, "masks")


@pytest.fixture(scope="module")
def masks():
    return pkg_module("masks")


def ann_of(seg, id=1, iscrowd=0, num_keypoints=9, area=5000.0):
    return dict(id=id, iscrowd=iscrowd, num_keypoints=num_keypoints, area=area, segmentation=seg)


# ---- the polygon set shared with tests/test_gpu_masks.py ----
def polygon_set(count=330, seed=20250317):
    """[(h, w, xy)]: three kinds in turn -- random points partly outside the image, two-decimal
    coordinates inside, star-shaped around a centre -- with 3 .. 11 points, sizes 8 .. 70.  The first
    two kinds are mostly self-intersecting."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        h, w = int(rng.integers(8, 71)), int(rng.integers(8, 71))
        k = int(rng.integers(3, 12))
        if i % 3 == 0:
            xy = rng.uniform(-0.3, 1.3, (k, 2)) * [w, h]
        elif i % 3 == 1:
            xy = np.round(rng.uniform(0, 1, (k, 2)) * [w, h], 2)
        else:
            ang = np.sort(rng.uniform(0, 2 * np.pi, k))
            rad = rng.uniform(0.15, 0.6, k) * min(h, w)
            c = rng.uniform(0.3, 0.7, 2) * [w, h]
            xy = c + np.stack([np.cos(ang), np.sin(ang)], axis=1) * rad[:, None]
        out.append((h, w, np.ascontiguousarray(xy, np.float64).ravel()))
    return out


def crossing_number(xy, h, w):
    """An independent float64 even-odd test at the pixel centres (c + 0.5, r + 0.5) and every
    centre's distance to the nearest edge: (inside (h, w) bool, distance (h, w))."""
    p = np.asarray(xy, np.float64).reshape(-1, 2)
    q = np.roll(p, -1, axis=0)
    py, px = np.mgrid[0:h, 0:w].astype(np.float64) + 0.5
    inside = np.zeros((h, w), bool)
    dist = np.full((h, w), np.inf)
    for (x0, y0), (x1, y1) in zip(p, q):
        if (y0 > y1):
            (x0, y0), (x1, y1) = (x1, y1), (x0, y0)
        if y0 != y1:
            hit = (py >= y0) & (py < y1)
            xc = x0 + (py - y0) * (x1 - x0) / (y1 - y0)
            inside ^= hit & (xc > px)
        ex, ey = x1 - x0, y1 - y0
        ll = ex * ex + ey * ey
        t = np.clip(((px - x0) * ex + (py - y0) * ey) / ll, 0, 1) if ll > 0 else np.zeros((h, w))
        dist = np.minimum(dist, np.hypot(px - (x0 + t * ex), py - (y0 + t * ey)))
    return inside, dist


RLE_CASES = [  # (h, w, counts)
    (3, 4, [0, 3, 0, 2, 7]),            # a leading zero count and a zero-length run inside
    (5, 7, [4, 0, 0, 6, 3, 0, 2, 20]),  # two zero-length runs in a row: the toggles cancel
    (6, 5, [30]),                       # all zeros
    (6, 5, [0, 30]),                    # all ones: the last toggle is h * w
    (37, 53, [100, 37, 500, 3, 0, 1, 1320]),
]


def rle_want(h, w, counts):
    flat = np.concatenate([np.full(c, k % 2, np.uint8) for k, c in enumerate(counts)])
    return flat.reshape(w, h).T.astype(bool)


# ---- 1. gen_masks against the reference's own function ----
def test_gen_fixtures_cover_the_cases():
    names = sorted(os.path.basename(p)[4:-4] for p in glob.glob(os.path.join(MASKS, "gen_*.npz")))
    assert names == ["crowd_crowd", "crowd_first", "crowd_last", "mixed", "none", "thresholds"]
    first, last = np.load(os.path.join(MASKS, "gen_crowd_first.npz")), np.load(os.path.join(MASKS, "gen_crowd_last.npz"))
    assert np.array_equal(first["masks"][0], last["masks"][1]) and np.array_equal(first["masks"][1], last["masks"][0])
    assert np.array_equal(first["mask_all"], last["mask_all"]) and not np.array_equal(first["mask_miss"], last["mask_miss"])
    th = np.load(os.path.join(MASKS, "gen_thresholds.npz"))
    assert th["num_keypoints"].tolist() == [4, 5, 9, 9] and th["area"].tolist() == [5000.0, 5000.0, 1024.0, 1025.0]
    assert len(np.load(os.path.join(MASKS, "gen_none.npz"))["masks"]) == 0


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(MASKS, "gen_*.npz"))), ids=os.path.basename)
def test_gen_masks_np_equals_the_reference(masks, path):
    d = np.load(path)
    anns = [dict(iscrowd=int(c), num_keypoints=int(k), area=float(a))
            for c, k, a in zip(d["iscrowd"], d["num_keypoints"], d["area"])]
    h, w = d["mask_all"].shape
    mask_all, mask_miss = masks.gen_masks_np(anns, h, w, masks=d["masks"])
    assert mask_all.dtype == bool and mask_miss.dtype == bool
    assert np.array_equal(mask_all, d["mask_all"]) and np.array_equal(mask_miss, d["mask_miss"])


# ---- 2. the rasteriser's statement ----
@pytest.mark.parametrize("x,y,bw,bh,h,w", [(2, 3, 8, 5, 12, 14), (0, 0, 5, 4, 4, 5), (3, 0, 1, 1, 6, 9), (0, 2, 7, 3, 5, 7)])
def test_integer_rectangles_fill_exactly(masks, x, y, bw, bh, h, w):
    got = masks.ann_to_mask_np(ann_of([[x, y, x + bw, y, x + bw, y + bh, x, y + bh]]), h, w)
    want = np.zeros((h, w), bool)
    want[y:y + bh, x:x + bw] = True
    assert np.array_equal(got, want)


def test_polygons_agree_with_the_crossing_number_outside_a_one_pixel_band(masks):
    polys = polygon_set()
    assert len(polys) >= 300
    worst, differ, pixels = 0.0, 0, 0
    for h, w, xy in polys:
        got = masks.toggles_to_mask(masks.poly_toggles(xy, h, w), h, w)
        inside, dist = crossing_number(xy, h, w)
        bad = got != inside
        if bad.any():
            worst = max(worst, float(dist[bad].max()))
        differ += int(bad.sum())
        pixels += h * w
    print("worst disagreeing pixel %.3f px from an edge; %d of %d pixels differ (%.2f %%)" % (
        worst, differ, pixels, 100.0 * differ / pixels))
    assert worst <= 1.0


# ---- 3. other statement cases ----
@pytest.mark.parametrize("h,w,counts", RLE_CASES)
def test_rle(masks, h, w, counts):
    toggles = masks.rle_toggles(counts, h, w)
    assert toggles[-1] == h * w
    assert np.array_equal(masks.toggles_to_mask(toggles, h, w), rle_want(h, w, counts))
    assert np.array_equal(masks.ann_to_mask_np(ann_of(dict(size=[h, w], counts=counts), iscrowd=1), h, w),
                          rle_want(h, w, counts))


def test_rle_errors(masks):
    with pytest.raises(ValueError):
        masks.rle_toggles([0, 3, 0, 2, 6], 3, 4)
    with pytest.raises(ValueError):
        masks.rle_toggles([12], 3, 4, size=[4, 3])
    with pytest.raises(ValueError, match="77"):
        masks.ann_to_mask_np(ann_of(dict(size=[3, 4], counts=[5, 8]), id=77), 3, 4)
    with pytest.raises(ValueError, match="77"):
        masks.ann_to_mask_np(ann_of(dict(size=[4, 3], counts=[5, 7]), id=77), 3, 4)


def test_two_polygons_are_the_union(masks):
    a, b = [2.5, 1.0, 20.0, 3.0, 12.5, 18.0], [10.0, 10.0, 28.0, 12.0, 26.0, 29.5, 8.0, 25.0]
    one = masks.ann_to_mask_np(ann_of([a]), 32, 30)
    two = masks.ann_to_mask_np(ann_of([b]), 32, 30)
    assert (one & two).any() and (one ^ two).any()
    assert np.array_equal(masks.ann_to_mask_np(ann_of([a, b]), 32, 30), one | two)
    assert not masks.ann_to_mask_np(ann_of([]), 32, 30).any()


@pytest.mark.parametrize("box,rows,cols", [
    ((-5, 4, 6, 9), (4, 9), (0, 6)),        # over the left side
    ((10, -7, 40, 3), (0, 3), (10, 20)),    # over the top and the right side
    ((3, 10, 8, 99), (10, 16), (3, 8)),     # over the bottom
    ((-9, -9, 99, 99), (0, 16), (0, 20)),   # over every side
])
def test_polygons_are_clipped_at_the_image(masks, box, rows, cols):
    x0, y0, x1, y1 = box
    got = masks.ann_to_mask_np(ann_of([[x0, y0, x1, y0, x1, y1, x0, y1]]), 16, 20)
    want = np.zeros((16, 20), bool)
    want[rows[0]:rows[1], cols[0]:cols[1]] = True
    assert np.array_equal(got, want)


@pytest.mark.parametrize("poly", [[-30, 2, -4, 3, -10, 12], [25, 2, 44, 3, 30, 12], [2, -30, 12, -4, 5, -9],
                                  [2, 20, 12, 44, 5, 30], [300, 300, 340, 310, 320, 390]])
def test_a_polygon_outside_the_image_is_empty(masks, poly):
    assert not masks.ann_to_mask_np(ann_of([poly]), 16, 20).any()


@pytest.mark.parametrize("seg,word", [
    (dict(size=[16, 20], counts="0e4f"), "compressed"),
    ([[1, 2, 3, 4, 5, 6, 7]], "polygon"),
    ([[1, 2, 3, 4]], "polygon"),
    ([[1, 2, 9, 4, 5, float("nan")]], "coordinate"),
    ([[1, 2, 9, 4, 5, float("inf")]], "coordinate"),
    ([[1, 2, 9, 4, 5, 65536.5]], "coordinate"),
    ([[1, 2, 9, 4, -65537, 8]], "coordinate"),
])
def test_declared_limits_raise_naming_the_annotation(masks, lib, seg, word):
    for call in (lambda a: masks.ann_to_mask_np(a, 16, 20), lambda a: lib.pack_annotations([(16, 20, [a])])):
        with pytest.raises(ValueError) as e:
            call(ann_of(seg, id=4711))
        assert "4711" in str(e.value) and word in str(e.value)
    # the largest magnitude allowed passes
    masks.ann_to_mask_np(ann_of([[1, 2, 9, 4, 65536, -65536]]), 16, 20)


# ---- 4. pack_annotations ----
def hand_made():
    return [
        (10, 12, [ann_of([[1, 1, 8, 1, 8, 8], [2.5, 3, 9, 4, 5, 9.25, 1, 7]], id=1),
                  ann_of(dict(size=[10, 12], counts=[7, 20, 93]), id=2, iscrowd=1, num_keypoints=0)]),
        (6, 5, []),
        (8, 9, [ann_of([], id=3, num_keypoints=4), ann_of([[0, 0, 4, 0, 4, 4]], id=4, area=1024.0),
                ann_of([[0, 0, 4, 0, 4, 4]], id=5, num_keypoints=5, area=1025.0)]),
    ]


def test_pack_annotations_round_trips(masks, lib):
    images = hand_made()
    p = lib.pack_annotations(images)
    assert p["hw"].tolist() == [10, 12, 6, 5, 8, 9] and p["hw"].dtype == np.int32
    assert p["ann_offsets"].tolist() == [0, 2, 2, 5]
    assert p["part_offsets"].tolist() == [0, 2, 3, 3, 4, 5]
    assert p["part_kind"].tolist() == [0, 0, 1, 0, 0]
    assert p["data_offsets"].tolist() == [0, 6, 14, 17, 23, 29] and p["data_offsets"].dtype == np.int64
    assert p["xy"].dtype == np.float64 and p["counts"].dtype == np.uint32 and len(p["xy"]) == len(p["counts"]) == 29
    back = []  # the segmentations read back out of the flat arrays
    for a in range(p["ann_offsets"][-1]):
        parts = []
        for q in range(p["part_offsets"][a], p["part_offsets"][a + 1]):
            lo, hi = p["data_offsets"][q], p["data_offsets"][q + 1]
            parts.append(p["xy"][lo:hi].tolist() if p["part_kind"][q] == 0 else p["counts"][lo:hi].tolist())
        back.append(parts)
    anns = [a for _, _, anns in images for a in anns]
    want = [[[float(v) for v in poly] for poly in a["segmentation"]] if isinstance(a["segmentation"], list)
            else [a["segmentation"]["counts"]] for a in anns]
    assert back == want
    # roles: crowd; too few keypoints; area at the threshold; just over both thresholds
    assert p["ann_role"].tolist() == [0, 2, 1, 1, 0] == [masks.ann_role(a) for a in anns]
    for h, w, anns in images:  # the roles are gen_masks_np's: the same masks either way
        by_role = {0: (True, False), 1: (True, True)}
        for a in anns:
            m = masks.ann_to_mask_np(a, h, w)
            if m.any() and not a["iscrowd"]:
                got = masks.gen_masks_np([a], h, w)
                assert (got[0].any(), got[1].any()) == by_role[masks.ann_role(a)]


def test_tiny_coco_fixture(masks):
    gen = pkg_module("gen_ignore_mask")
    labels = pkg_module("labels")
    images = gen.load_images(os.path.join(MASKS, "tiny_coco.json"))
    assert [i[0] for i in images] == [139, 285, 632] and [len(i[3]) for i in images] == [3, 2, 3]
    miss = [masks.gen_masks_np(anns, h, w)[1].any() for _, h, w, anns in images]
    assert miss == [True, False, True]  # the second image writes no PNG
    assert [labels.valid_annotations(i[3]) is not None for i in images] == [True, True, False]
    assert sum(isinstance(a["segmentation"], dict) for i in images for a in i[3]) == 1
    with open(os.path.join(MASKS, "tiny_coco.json")) as f:
        assert len(json.load(f)["annotations"]) == 8


# ---- 7. the argument checks of op_ignore_masks (before any device call: no device needed) ----
def _call(lib, p, n=None, drop=(), outs=None):
    def arg(name):
        return None if name in drop or not p[name].size else lib.ptr(p[name])

    n = len(p["hw"]) // 2 if n is None else n
    keep = [np.zeros((max(int(p["hw"][2 * f]), 1), max(int(p["hw"][2 * f + 1]), 1)), np.uint8) for f in range(len(p["hw"]) // 2)]
    tab = (ctypes.c_void_p * len(keep))(*[a.ctypes.data for a in keep])
    rc = lib.lib().op_ignore_masks(0, n, arg("hw"), arg("ann_offsets"), arg("ann_role"), arg("part_offsets"),
                                   arg("part_kind"), arg("data_offsets"), arg("xy"), arg("counts"), tab, None, None)
    return rc, lib.last_error()


def test_op_ignore_masks_rejects_bad_arguments(masks, lib):
    """Every check runs before the first device call: this passes on a machine without a device."""
    def good():
        return lib.pack_annotations(hand_made())

    def bad(word, edit=None, **kw):
        p = good()
        if edit:
            edit(p)
        rc, msg = _call(lib, p, **kw)
        assert rc == lib.OP_ERR_INVALID and "op_ignore_masks" in msg and word in msg, (word, rc, msg)

    def put(name, index, value):
        def edit(p):
            p[name][index] = value
        return edit

    bad("n must", n=0)
    bad("n must", n=-3)
    for name in ("hw", "ann_offsets", "ann_role", "part_offsets", "part_kind", "data_offsets", "xy", "counts"):
        bad("null " + name, drop=(name,))
    for index, value in ((0, 0), (1, 0), (2, -1), (3, 16385), (4, 16385)):
        bad("hw", put("hw", index, value))
    bad("ann_offsets", put("ann_offsets", 0, 1))
    bad("ann_offsets", put("ann_offsets", 1, 3))   # 0 3 2 5: decreases
    bad("part_offsets", put("part_offsets", 0, 1))
    bad("part_offsets", put("part_offsets", 2, 1))
    bad("data_offsets", put("data_offsets", 0, 2))
    bad("data_offsets", put("data_offsets", 3, 13))
    bad("ann_role", put("ann_role", 1, 3))
    bad("ann_role", put("ann_role", 0, -1))
    bad("part_kind", put("part_kind", 4, 2))
    bad("xy", put("data_offsets", 1, 5))            # an odd polygon (and the next one too)
    bad("xy", put("data_offsets", 4, 19))           # a polygon of two points
    for value in (np.nan, np.inf, -np.inf, 65536.5, -70000.0):
        bad("xy", put("xy", 9, value))
    bad("counts", put("counts", 15, 21))            # the runs sum to 121 on a 10 x 12 image
    bad("counts", put("hw", 0, 11))
    bad("part 3", put("xy", 18, np.nan))            # a later part is checked too, and named
    ms = ctypes.c_double()
    assert lib.lib().op_ignore_masks_last_ms(0, None) == lib.OP_ERR_INVALID
    assert lib.lib().op_ignore_masks_last_ms(-1, ctypes.byref(ms)) == lib.OP_ERR_INVALID
    assert lib.lib().op_ignore_masks_last_ms(64, ctypes.byref(ms)) == lib.OP_ERR_INVALID
