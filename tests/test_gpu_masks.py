"""Ignore masks from COCO segmentations on the device (op_ignore_masks, csrc/masks.hip):
every mask equals masks.py's NumPy statement bit for bit."""
import os
import random

import numpy as np
import pytest

from conftest import pkg_module
from test_masks_host import MASKS, RLE_CASES, ann_of, polygon_set

pytestmark = pytest.mark.gpu

# h x w; 700 x 40: a tall column (22 toggle words each); 1100 x 130: column blocks of 59 columns, which
# start inside a toggle word and inside a word of the column bits
SIZES = [(1, 1), (1, 40), (37, 53), (33, 31), (64, 96), (31, 1), (700, 40), (1100, 130)]


@pytest.fixture(scope="module")
def masks():
    return pkg_module("masks")


def polygons_for(h, w, rng):
    """Polygons on an h x w image: the shared set's shapes stretched to this size, a triangle, one of
    about 200 points, repeated vertices (zero-length edges) and vertices far outside (+-300)."""
    out = []
    for ph, pw, xy in polygon_set(count=12, seed=h * 1000 + w):
        out.append((xy.reshape(-1, 2) * [w / pw, h / ph]).ravel())
    out.append(np.array([0.2 * w, 0.1 * h, 0.9 * w, 0.5 * h, 0.3 * w, 0.95 * h]))
    ang = np.linspace(0, 2 * np.pi, 200, endpoint=False)
    rad = (0.3 + 0.15 * np.sin(7 * ang) + 0.02 * rng.random(200)) * min(h, w)
    out.append((np.stack([w / 2 + rad * np.cos(ang), h / 2 + rad * np.sin(ang)], axis=1)).ravel())
    tri = np.array([[0.1 * w, 0.2 * h], [0.8 * w, 0.3 * h], [0.4 * w, 0.9 * h]])
    out.append(tri[[0, 0, 1, 1, 1, 2, 0]].ravel())
    out.append(np.array([-300.0, -250.0, 300.0, 0.4 * h, 0.6 * w, 300.0, -300.0, 280.0, 0.5 * w, 0.5 * h]))
    out.append(np.array([-300.0, 0.3 * h, 300.0, 0.3 * h + 0.4, 300.0, 0.8 * h, -300.0, 0.8 * h - 0.3]))
    return [np.ascontiguousarray(p, np.float64) for p in out]


@pytest.mark.parametrize("h,w", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_out_ann_equals_ann_to_mask_np(masks, lib, h, w):
    """One call per size: every polygon as an annotation of its own, then all of them as the parts
    of one annotation (the union), through out_ann."""
    polys = polygons_for(h, w, np.random.default_rng(h * 7 + w))
    anns = [ann_of([p.tolist()], id=k) for k, p in enumerate(polys)]
    anns.append(ann_of([p.tolist() for p in polys[:6]], id=len(polys)))
    want = [masks.ann_to_mask_np(a, h, w) for a in anns]
    per = [np.full((h, w), 7, np.uint8) for _ in anns]
    lib.ignore_masks_call(0, 1, lib.pack_annotations([(h, w, anns)]), None, None, per)
    for k, (g, v) in enumerate(zip(per, want)):
        assert g.max() <= 1 and np.array_equal(g.astype(bool), v), (k, int((g.astype(bool) != v).sum()))
    if h * w > 100:
        assert sum(int(v.sum()) for v in want) > h * w // 4  # the cases are not empty
    assert np.array_equal(masks.ann_to_mask(anns[1], h, w), want[1])


def test_shared_polygon_set_on_the_device(masks, lib):
    """The polygons of the host test (tests/test_masks_host.py), each on its own image, in one call."""
    polys = polygon_set()
    images = [(h, w, [ann_of([xy.tolist()], id=k)]) for k, (h, w, xy) in enumerate(polys)]
    per = [np.empty((h, w), np.uint8) for h, w, _ in images]
    lib.ignore_masks_call(0, len(images), lib.pack_annotations(images), None, None, per)
    for (h, w, anns), g in zip(images, per):
        assert np.array_equal(g.astype(bool), masks.ann_to_mask_np(anns[0], h, w)), anns[0]["id"]


@pytest.mark.parametrize("h,w,counts", RLE_CASES)
def test_rle_on_the_device(masks, h, w, counts):
    ann = ann_of(dict(size=[h, w], counts=counts), iscrowd=1)
    assert np.array_equal(masks.ann_to_mask(ann, h, w), masks.ann_to_mask_np(ann, h, w))


def test_long_rle_on_the_device(masks):
    """More runs than one scan chunk of the kernel holds (256), zero-length runs among them."""
    rng = np.random.default_rng(5)
    h, w = 64, 96
    counts = rng.integers(0, 12, 900)
    counts = counts[np.cumsum(counts) <= h * w].tolist()
    counts.append(h * w - sum(counts))
    assert len(counts) > 600 and 0 in counts[1:-1]
    ann = ann_of(dict(size=[h, w], counts=counts), iscrowd=1)
    assert np.array_equal(masks.ann_to_mask(ann, h, w), masks.ann_to_mask_np(ann, h, w))


def batch_images():
    """5 images of different sizes, 0 .. 12 annotations each, mixed roles and kinds."""
    rng = np.random.default_rng(11)
    images, next_id = [], 1
    for (h, w), count in zip([(37, 53), (64, 96), (20, 17), (33, 31), (90, 41)], [12, 7, 0, 5, 9]):
        anns = []
        for k in range(count):
            role = (k + h) % 3
            if role == 2 and k % 2 == 0:  # a crowd as an RLE: a few runs
                counts = rng.integers(0, h * w // 6, 8)
                counts = counts[np.cumsum(counts) <= h * w].tolist()
                seg = dict(size=[h, w], counts=counts + [h * w - sum(counts)])
            else:
                seg = []
                for _ in range(int(rng.integers(1, 3))):
                    c = rng.uniform(0.1, 0.9, 2) * [w, h]
                    ang = np.sort(rng.uniform(0, 2 * np.pi, int(rng.integers(3, 9))))
                    rad = rng.uniform(0.1, 0.5, len(ang)) * min(h, w)
                    seg.append(np.round(c + np.stack([np.cos(ang), np.sin(ang)], axis=1) * rad[:, None], 2).ravel().tolist())
            anns.append(ann_of(seg, id=next_id, iscrowd=int(role == 2), num_keypoints=3 if role == 1 else 8,
                               area=900.0 if role == 1 and k % 2 else 3000.0))
            next_id += 1
        images.append((h, w, anns))
    return images


def test_ignore_masks_equals_gen_masks_np(masks):
    images = batch_images()
    assert [len(a) for _, _, a in images] == [12, 7, 0, 5, 9]
    got = masks.ignore_masks(images)
    assert masks.last_ms(0) > 0
    for (h, w, anns), (mask_all, mask_miss) in zip(images, got):
        want_all, want_miss = masks.gen_masks_np(anns, h, w)
        assert mask_all.dtype == bool and np.array_equal(mask_all, want_all), (h, w)
        assert np.array_equal(mask_miss, want_miss), (h, w)
    assert sum(int(m.sum()) for _, m in got) > 500 and not got[2][0].any()
    assert any((a & ~m).any() for a, m in got)
    # each image alone, and the batch a second time: the same bytes
    for image, (mask_all, mask_miss) in zip(images, got):
        (one_all, one_miss), = masks.ignore_masks([image])
        assert np.array_equal(one_all, mask_all) and np.array_equal(one_miss, mask_miss)
    again = masks.ignore_masks(images)
    for (a0, m0), (a1, m1) in zip(got, again):
        assert a0.tobytes() == a1.tobytes() and m0.tobytes() == m1.tobytes()


def tiny_coco():
    return pkg_module("gen_ignore_mask").load_images(os.path.join(MASKS, "tiny_coco.json"))


def test_update_annotated_equals_update_samples_on_gen_masks_np(masks, rand_weights):
    train = pkg_module("train")
    (_, h0, w0, anns0), (_, h1, w1, anns1), (_, h2, w2, anns2) = tiny_coco()
    rng = np.random.default_rng(3)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((h0, w0), (h1, w1), (h2, w2))]
    labels = pkg_module("labels")
    n, insize = 2, 64
    out = []
    for chained in (True, False):
        up = train.Updater(n, insize, insize, model=rand_weights, resume=True)
        try:
            py, npr = random.Random(5), np.random.RandomState(5)
            if chained:
                loss = up.update_annotated([(imgs[0], anns0), (imgs[1], anns1)], py, npr)
                with pytest.raises(ValueError, match="sample 1"):
                    up.update_annotated([(imgs[0], anns0), (imgs[2], anns2)], py, npr)
            else:
                samples = [(img, masks.gen_masks_np(anns, img.shape[0], img.shape[1])[1],
                            labels.parse_coco_annotation(labels.valid_annotations(anns)))
                           for img, anns in ((imgs[0], anns0), (imgs[1], anns1))]
                assert samples[0][1].any()
                loss = up.update_samples(samples, py, npr)
            out.append((loss, up.weights()))
        finally:
            up.ctx.close()
    (l0, w0_), (l1, w1_) = out
    assert l0[0] > 0 and len(l0[1]) == 6 and len(l0[2]) == 6 and l0 == l1  # the twelve losses
    for name in w0_:
        for k in (0, 1):
            assert np.array_equal(w0_[name][k], w1_[name][k]), name
    assert any(not np.array_equal(w0_[name][0], rand_weights[name][0]) for name in w0_)


def test_cli_writes_the_reference_png_tree(masks, tmp_path):
    from PIL import Image
    gen = pkg_module("gen_ignore_mask")
    path = os.path.join(MASKS, "tiny_coco.json")
    out = tmp_path / "ignore_mask_val2017"
    assert gen.main(["--annotations", path, "--out", str(out), "--batch", "2"]) == 0
    want = {}
    for img_id, h, w, anns in gen.load_images(path):
        miss = masks.gen_masks_np(anns, h, w)[1]
        if miss.any():
            want["%012d.png" % img_id] = miss.astype(np.uint8) * 255
    assert sorted(os.listdir(out)) == sorted(want) == ["000000000139.png", "000000000632.png"]
    for name, pixels in want.items():
        img = Image.open(out / name)
        assert img.mode == "L" and np.array_equal(np.asarray(img), pixels), name
