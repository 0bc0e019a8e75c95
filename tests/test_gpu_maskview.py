"""The --vis viewer of gen_ignore_mask.py on the device (op_annotation_views, csrc/maskview.hip):
every byte equals maskview.py's NumPy statement, nothing excluded."""
import glob
import os
import time

import numpy as np
import pytest

from conftest import pkg_module
from test_masks_host import MASKS, ann_of
from test_maskview_host import VIEWS, fixture_anns

pytestmark = pytest.mark.gpu

# h x w: (16, 64) is exactly one tile, (17, 65) one pixel over in both directions; 3 w is a multiple of 4
# (rows start on a dword) for (16, 64) and (64, 96) and is not for (1, 1), (17, 65) and (37, 53)
SIZES = [(1, 1), (16, 64), (17, 65), (37, 53), (64, 96)]


@pytest.fixture(scope="module")
def mv():
    return pkg_module("maskview")


def rle_of(mask):
    """An (h, w) mask as an uncompressed COCO RLE (column-major runs, 0s first)."""
    flat = np.asarray(mask).astype(bool).T.ravel()
    edges = np.flatnonzero(np.diff(flat.astype(np.int8))) + 1
    counts = np.diff(np.concatenate([[0], edges, [flat.size]])).tolist()
    if flat[0]:
        counts = [0] + counts
    return dict(size=[int(mask.shape[0]), int(mask.shape[1])], counts=[int(c) for c in counts])


def frame_of(rng, h, w):
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    img[h // 3] = 0
    img[(2 * h) // 3] = 255
    return img


def keypoints_for(rng, h, w, count):
    """(x, y, v) triples: inside, on and over every border, v in {0, 1, 2}."""
    kp = np.stack([rng.integers(-4, w + 4, count), rng.integers(-4, h + 4, count), rng.integers(0, 3, count)], axis=1)
    return [int(v) for v in kp.ravel()]


def annotations_for(rng, h, w, count, first_id=1):
    """Mixed roles and kinds as test_gpu_masks.batch_images builds them, plus keypoints."""
    anns = []
    for k in range(count):
        role = (k + h) % 3
        if role == 2 and k % 2 == 0:  # a crowd as an RLE: a few runs
            counts = rng.integers(0, max(h * w // 6, 1), 8)
            counts = counts[np.cumsum(counts) <= h * w].tolist()
            seg = dict(size=[h, w], counts=[int(c) for c in counts] + [h * w - int(sum(counts))])
        else:
            seg = []
            for _ in range(int(rng.integers(1, 3))):  # one or two polygons: multi-part
                c = rng.uniform(0.1, 0.9, 2) * [w, h]
                ang = np.sort(rng.uniform(0, 2 * np.pi, int(rng.integers(3, 9))))
                rad = rng.uniform(0.2, 0.7, len(ang)) * max(min(h, w), 2)
                seg.append(np.round(c + np.stack([np.cos(ang), np.sin(ang)], axis=1) * rad[:, None], 2).ravel().tolist())
        ann = ann_of(seg, id=first_id + k, iscrowd=int(role == 2), num_keypoints=0 if role == 1 else 8,
                     area=900.0 if role == 1 and k % 2 else 3000.0)
        ann["keypoints"] = keypoints_for(rng, h, w, 17)
        anns.append(ann)
    return anns


def assert_views(mv, samples, got=None):
    got = mv.views(samples) if got is None else got
    assert len(got) == len(samples)
    for f, ((img, anns), (ann_img, msk_img)) in enumerate(zip(samples, got)):
        want_ann, want_msk = mv.view_np(img, anns)
        assert ann_img.dtype == np.uint8 and ann_img.shape == np.asarray(img).shape
        assert np.array_equal(ann_img, want_ann), (f, np.argwhere((ann_img != want_ann).any(axis=2))[:8])
        assert np.array_equal(msk_img, want_msk), (f, np.argwhere((msk_img != want_msk).any(axis=2))[:8])
    return got


# ---- the fixtures of the reference's own code, their masks as RLE segmentations ----
@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(VIEWS, "ann_*.npz"))), ids=os.path.basename)
def test_annotation_fixtures_on_the_device(mv, path):
    d = np.load(path)
    anns = fixture_anns(d)
    for ann, mask in zip(anns, d["masks"]):
        ann["segmentation"] = rle_of(mask)
    (ann_img, _), = assert_views(mv, [(d["frame"], anns)])
    assert np.array_equal(ann_img, d["out"])  # the reference's own picture


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(VIEWS, "gen_*.npz"))), ids=os.path.basename)
def test_mask_miss_fixtures_on_the_device(mv, path):
    d = np.load(path)
    ann = ann_of(rle_of(d["mask"]), id=1, num_keypoints=2)  # too few keypoints: its mask is mask_miss
    ann["keypoints"] = []
    (_, msk_img), = assert_views(mv, [(d["frame"], [ann])])
    assert np.array_equal(msk_img, d["out"])


# ---- sizes ----
@pytest.mark.parametrize("h,w", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_views_equal_view_np(mv, h, w):
    rng = np.random.default_rng(h * 100 + w)
    anns = annotations_for(rng, h, w, 9)
    assert any(isinstance(a["segmentation"], dict) for a in anns) and any(isinstance(a["segmentation"], list) and len(a["segmentation"]) == 2 for a in anns)
    img = frame_of(rng, h, w)
    (ann_img, msk_img), = assert_views(mv, [(img, anns)])
    if h * w > 100:
        assert (ann_img != img).mean() > 0.3 and (msk_img != img).any()


def test_a_batch_of_five_sizes_in_one_call(mv):
    rng = np.random.default_rng(21)
    samples, next_id = [], 1
    for (h, w), count in zip([(37, 53), (64, 96), (20, 17), (33, 131), (90, 41)], [12, 7, 0, 5, 9]):
        samples.append((frame_of(rng, h, w), annotations_for(rng, h, w, count, next_id)))
        next_id += count
    got = assert_views(mv, samples)
    assert mv.last_ms(0) > 0
    assert np.array_equal(got[2][0], samples[2][0]) and np.array_equal(got[2][1], samples[2][0])  # no annotations
    # each image alone, and the batch a second time: the same bytes
    for sample, (ann_img, msk_img) in zip(samples, got):
        (one_ann, one_msk), = mv.views([sample])
        assert np.array_equal(one_ann, ann_img) and np.array_equal(one_msk, msk_img)
    for (a0, m0), (a1, m1) in zip(got, mv.views(samples)):
        assert a0.tobytes() == a1.tobytes() and m0.tobytes() == m1.tobytes()


def test_a_strided_frame(mv):
    rng = np.random.default_rng(22)
    h, w = 37, 53
    big = rng.integers(0, 256, (h + 6, w + 20, 3), dtype=np.uint8)
    view = big[3:3 + h, 7:7 + w]
    assert view.strides[0] > 3 * w and not view.flags.c_contiguous
    anns = annotations_for(rng, h, w, 6)
    assert mv.pack_views([(view, anns)])[1]["row_stride"].tolist() == [big.strides[0]]
    got = assert_views(mv, [(view, anns)])
    assert_views(mv, [(np.ascontiguousarray(view), anns)], got)


def test_an_annotation_with_300_keypoints(mv):
    """More discs than one cull chunk of the kernel holds (256); they overlap, so the order matters."""
    rng = np.random.default_rng(23)
    h, w = 64, 96
    anns = annotations_for(rng, h, w, 3)
    kp = np.stack([rng.integers(-3, w + 3, 300), rng.integers(-3, h + 3, 300), rng.integers(1, 3, 300)], axis=1)
    kp[250:262, :2] = [40, 30]  # a stack of discs on one centre across the chunk boundary, alternating colours
    kp[250:262, 2] = [1, 2] * 6
    kp[299] = (70, 20, 1)
    kp[3] = (70, 21, 2)
    anns[1]["keypoints"] = [int(v) for v in kp.ravel()]
    img = frame_of(rng, h, w)
    assert_views(mv, [(img, anns)])
    swapped = [dict(a) for a in anns]
    swapped[1]["keypoints"] = [int(v) for v in kp[::-1].ravel()]
    assert not np.array_equal(mv.view_np(img, swapped)[0], mv.view_np(img, anns)[0])


def test_an_annotation_whose_mask_is_empty(mv):
    rng = np.random.default_rng(24)
    h, w = 37, 53
    empty = ann_of([], id=1)
    empty["keypoints"] = [10, 10, 1, 30, 20, 2]
    outside = ann_of([[300, 300, 340, 310, 320, 390]], id=2, iscrowd=1)
    outside["keypoints"] = []
    img = frame_of(rng, h, w)
    (ann_img, msk_img), = assert_views(mv, [(img, [empty, outside])])
    assert np.array_equal(msk_img, img) and 0 < (ann_img != img).any(axis=2).sum() <= 2 * 29


def test_one_output_only(mv):
    rng = np.random.default_rng(25)
    samples = [(frame_of(rng, h, w), annotations_for(rng, h, w, 5)) for h, w in ((37, 53), (16, 64))]
    both = assert_views(mv, samples)
    only_ann = mv.views(samples, want_miss=False)
    only_miss = mv.views(samples, want_ann=False)
    for (a, m), (a1, m1), (a2, m2) in zip(both, only_ann, only_miss):
        assert m1 is None and a2 is None and np.array_equal(a1, a) and np.array_equal(m2, m)
    # one entry left out: the other frames are filled, that one is untouched
    lib = pkg_module("_lib")
    frames, packed = mv.pack_views(samples)
    outs = [np.full(f.shape, 7, np.uint8) for f in frames]
    lib.annotation_views_call(0, frames, packed, [outs[0], None], [None, outs[1]])
    assert np.array_equal(outs[0], both[0][0]) and np.array_equal(outs[1], both[1][1])


def test_panels(mv):
    rng = np.random.default_rng(26)
    samples = [(frame_of(rng, 20, 33), annotations_for(rng, 20, 33, 4))]
    panel, = mv.panels(samples)
    assert panel.shape == (20, 66, 3) and np.array_equal(panel, mv.panel_np(*samples[0]))


def test_cli_writes_the_panels(mv, tmp_path):
    from PIL import Image
    gen = pkg_module("gen_ignore_mask")
    draw = pkg_module("draw")
    path = os.path.join(MASKS, "tiny_coco.json")
    rng = np.random.default_rng(27)
    images = gen.load_images(path, with_names=True)
    frames = tmp_path / "val2017"
    frames.mkdir()
    for img_id, h, w, anns, name in images:
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(frames / name)
    out = tmp_path / "vis"
    assert gen.main(["--annotations", path, "--out", str(out), "--vis", "--images", str(frames), "--batch", "2"]) == 0
    assert sorted(os.listdir(out)) == ["%012d.png" % i[0] for i in images]  # panels only: no mask PNG
    for img_id, h, w, anns, name in images:
        want = mv.panel_np(draw.read_bgr(str(frames / name)), anns)
        assert want.shape == (h, 2 * w, 3)
        assert np.array_equal(draw.read_bgr(str(out / ("%012d.png" % img_id))), want), img_id
    few = tmp_path / "few"
    assert gen.main(["--annotations", path, "--out", str(few), "--vis", "--images", str(frames), "--limit", "1"]) == 0
    assert os.listdir(few) == ["%012d.png" % images[0][0]]
    Image.fromarray(np.zeros((9, 9, 3), np.uint8)).save(frames / images[1][4])  # a frame of another size
    with pytest.raises(ValueError, match=str(images[1][0])):
        gen.main(["--annotations", path, "--out", str(few), "--vis", "--images", str(frames)])
    with pytest.raises(SystemExit):
        gen.main(["--annotations", path, "--out", str(few), "--vis"])


def test_timing_of_eight_frames(mv):
    """Prints the device time (op_annotation_views_last_ms: uploads, the mask kernels and the view kernel)
    and the host time of view_np on the same input: 8 frames of 368 x 368 with 8 annotations each.  No
    threshold: the device time is positive and the pictures are equal."""
    rng = np.random.default_rng(28)
    n, s = 8, 368
    samples = [(frame_of(rng, s, s), annotations_for(rng, s, s, 8, 1 + 8 * f)) for f in range(n)]
    mv.views(samples)  # first call: module load
    times = []
    for _ in range(5):
        got = mv.views(samples)
        times.append(mv.last_ms())
    t0 = time.perf_counter()
    want = [mv.view_np(*sample) for sample in samples]
    host_ms = (time.perf_counter() - t0) * 1e3
    for f in range(n):
        assert np.array_equal(got[f][0], want[f][0]) and np.array_equal(got[f][1], want[f][1]), f
    moved = n * 3 * s * s * 3  # the frame in, two pictures out
    print("\nop_annotation_views_last_ms (8 x 368 x 368, 8 annotations each): median %.3f ms, min %.3f, max %.3f of 5; "
          "view_np %.1f ms; %d bytes in and out" % (float(np.median(times)), min(times), max(times), host_ms, moved))
    assert min(times) > 0
