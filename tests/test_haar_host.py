"""haar.py on the host: the loader, the NumPy statement (scales, pyramid, integrals, the window test,
the stages, the skip rule, grouping) and face_demo's helpers.  The statement is the contract the
kernels are held to in test_gpu_haar.py; parity with OpenCV is not pinned (there is none to compare
with), so person.png is a sanity check with margins, not a parity test."""
import hashlib
import json
import math
import os

import numpy as np
import pytest

import haar_cases as cases
from conftest import pkg_module

H = cases.haar()


def test_loader_reads_the_reference_cascade():
    c = cases.real()
    assert np.diff(c["stage_first"]).tolist() == [3, 16, 21, 39, 33, 44, 50, 51, 56, 71, 80, 103, 111, 102, 135, 137, 140,
                                                   160, 177, 182, 211, 213]
    assert len(c["thr"]) == 2135 and c["win"].tolist() == [20, 20] and len(c["stage_thr"]) == 22
    assert c["rects"][0].tolist() == [[3, 7, 14, 4], [3, 9, 14, 2], [0, 0, 0, 0]]
    assert c["weights"][0].tolist() == [-1.0, 2.0, 0.0]
    assert c["thr"][0] == np.float32(4.0141958743333817e-03)
    assert c["left"][0] == np.float32(3.3794190734624863e-02) and c["right"][0] == np.float32(8.3781069517135620e-01)
    assert c["stage_thr"][0] == np.float32(0.82268941402435303) - np.float32(1e-5)
    for k in ("stage_thr", "weights", "thr", "left", "right"):
        assert c[k].dtype == np.float32, k
    assert (c["weights"][:, 2] != 0).any() and (c["weights"][:, 2] == 0).any()  # two- and three-rect features


def test_npz_round_trip_is_exact(tmp_path):
    for c in (cases.real(), cases.tiny()):
        path = str(tmp_path / "cascade.npz")
        H.save_cascade(path, c)
        back = H.load_cascade(path)
        assert sorted(back) == sorted(c)
        for k in c:
            assert back[k].dtype == c[k].dtype and np.array_equal(back[k], c[k]), k
    assert os.path.getsize(path) < 4096


@pytest.mark.parametrize("name, word", zip(cases.REFUSED, ("tilted", "stumps", "LBP", "HOG", "old-format", "65 x 5", "outside")))
def test_loader_refuses(name, word):
    with pytest.raises(ValueError, match=word):
        H.load_cascade(os.path.join(cases.DIR, name))


def test_integrals_against_a_double_loop():
    img = cases.noise(13, 17, 3)[:, :, 0].copy()
    s, q = H.integrals_np(img)
    assert s.dtype == np.int32 and q.dtype == np.uint32 and s.shape == q.shape == (14, 18)
    for y in range(14):
        for x in range(18):
            want_s = sum(int(img[j, i]) for j in range(y) for i in range(x))
            want_q = sum(int(img[j, i]) ** 2 for j in range(y) for i in range(x))
            assert s[y, x] == want_s and q[y, x] == want_q % 2 ** 32
    big = np.full((300, 300), 255, np.uint8)  # sqsum passes 2^32: kept modulo, window differences stay exact
    s, q = H.integrals_np(big)
    assert int(q[300, 300]) == (300 * 300 * 255 * 255) % 2 ** 32
    d = q[120:121, 120:121] - q[120:121, 102:103] - q[102:103, 120:121] + q[102:103, 102:103]  # arrays wrap silently
    assert int(d[0, 0]) == 18 * 18 * 255 * 255


def test_scales():
    got = H.scales(48, 64, (20, 20))
    assert [(lw, lh) for _, lw, lh in got] == [(64, 48), (53, 40), (44, 33), (37, 28), (31, 23)]
    assert [sc for sc, _, _ in got] == [np.float32(1.2 ** k) for k in range(5)] and got[0][0].dtype == np.float32
    assert [(lw, lh) for _, lw, lh in H.scales(20, 20, (20, 20))] == [(20, 20)]
    assert H.scales(30, 19, (20, 20)) == []
    assert [(lw, lh) for _, lw, lh in H.scales(48, 64, (20, 20), min_size=(30, 30))] == [(37, 28), (31, 23)]
    assert [(lw, lh) for _, lw, lh in H.scales(48, 64, (20, 20), max_size=(30, 30))] == [(64, 48), (53, 40), (44, 33)]
    for bad in (1.0, 1.009, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            H.scales(48, 64, (20, 20), bad)
    with pytest.raises(ValueError):
        H.scales(48, 64, (20, 20), min_size=(0, 1))
    with pytest.raises(ValueError):
        H.scales(3000, 3000, (20, 20), 1.01)  # more than 64 scales


def test_pyramid_at_factor_one_is_the_image_and_grey():
    img = cases.noise(31, 47, 5)
    g = H.grey_np(img)
    v = img.astype(np.int64)
    assert np.array_equal(g, (1868 * v[..., 0] + 9617 * v[..., 1] + 4899 * v[..., 2] + 8192) >> 14)
    assert np.array_equal(H.grey_np(g), g)  # 2-D: grey already
    assert np.array_equal(H.resize_np(g, 47, 31), g)
    layers = H.pyramid_np(img, cases.real())
    assert np.array_equal(layers[0]["pixels"], g) and layers[0]["step"] == 2
    flat = np.full((40, 50), 93, np.uint8)
    assert (H.resize_np(flat, 33, 27) == 93).all()  # weights sum to 256 * 256


def _walk(c, layer):
    """One rounded scalar operation at a time, positions in OpenCV's order, skip rule included."""
    f32 = np.float32
    win_w, win_h = int(c["win"][0]), int(c["win"][1])
    pix = layer["pixels"].astype(np.int64)
    n_stages = len(c["stage_thr"])
    area = (win_w - 2) * (win_h - 2)

    def rect(a, x, y, r):
        return int(a[y + r[1]:y + r[1] + r[3], x + r[0]:x + r[0] + r[2]].sum())

    m = np.full((len(layer["ys"]), len(layer["xs"])), -2, np.int8)
    step = layer["step"]
    for iy, y in enumerate(range(0, pix.shape[0] - win_h, step)):
        x = 0
        while x < pix.shape[1] - win_w:
            vs, vq = rect(pix, x, y, (1, 1, win_w - 2, win_h - 2)), rect(pix * pix, x, y, (1, 1, win_w - 2, win_h - 2))
            nf = float(area) * float(vq) - float(vs) * float(vs)
            res = -1
            if nf > 0:
                vnf = f32(1.0 / math.sqrt(nf))
                if f32(area) * vnf < f32(0.1):
                    res = n_stages
                    for k in range(n_stages):
                        total = f32(0)
                        for j in range(c["stage_first"][k], c["stage_first"][k + 1]):
                            w = c["weights"][j]
                            v = w[0] * f32(rect(pix, x, y, c["rects"][j][0])) + w[1] * f32(rect(pix, x, y, c["rects"][j][1]))
                            if w[2] != 0:
                                v = v + w[2] * f32(rect(pix, x, y, c["rects"][j][2]))
                            v = v * vnf
                            total = total + (c["left"][j] if v < c["thr"][j] else c["right"][j])
                        if total < c["stage_thr"][k]:
                            res = k
                            break
            m[iy, x // step] = res
            x += step
            if res == 0:
                x += step
    return m


def test_tiny_cascade_map_equals_a_scalar_walk():
    c = cases.tiny()
    assert np.diff(c["stage_first"]).tolist() == [3, 4] and c["win"].tolist() == [6, 5]
    maps, layers = H.result_map_np(cases.tiny_frame(), c)
    assert len(maps) == 13
    seen = set()
    for m, l in zip(maps, layers):
        assert m.dtype == np.int8 and np.array_equal(m, _walk(c, l))
        seen |= set(np.unique(m).tolist())
    assert seen == {-2, -1, 0, 1, 2}
    visited = np.concatenate([m.ravel() for m in maps])
    visited = visited[visited != -2]
    assert 0.3 < (visited == 0).mean() < 0.6 and 0.2 < (visited == 2).mean() < 0.45  # many survivors


def test_group_rectangles_hand_cases():
    g = H.group_rectangles_np
    # a chain: 0 ~ 1 and 1 ~ 2 but not 0 ~ 2 -> one class of three; its mean, rounded half to even
    chain = [(10, 10, 20, 20), (13, 10, 20, 20), (16, 10, 20, 20)]
    assert not H.similar_rects(chain[0], chain[2]) and H.similar_rects(chain[0], chain[1])
    r, n = g(chain, 2)
    assert r.tolist() == [[13, 10, 20, 20]] and n.tolist() == [3] and r.dtype == np.int32 and n.dtype == np.int32
    # a class of exactly min_neighbors members is dropped
    r, n = g(chain, 3)
    assert r.shape == (0, 4) and n.shape == (0,)
    # a small rect inside a strong one is dropped (n2 > max(3, n1)); the strong one stays
    strong = [(100, 100, 60, 60)] * 5 + [(120, 120, 12, 12)] * 4
    r, n = g(strong, 3)
    assert r.tolist() == [[100, 100, 60, 60]] and n.tolist() == [5]
    r, n = g([(100, 100, 60, 60)] * 4 + [(120, 120, 12, 12)] * 4, 3)  # equally strong: both stay
    assert r.tolist() == [[100, 100, 60, 60], [120, 120, 12, 12]] and n.tolist() == [4, 4]
    # classes are numbered by their first member
    r, n = g([(50, 50, 10, 10), (0, 0, 10, 10), (50, 50, 10, 10), (0, 0, 10, 10), (0, 1, 10, 10)], 1)
    assert r.tolist() == [[50, 50, 10, 10], [0, 0, 10, 10]] and n.tolist() == [2, 3]
    # min_neighbors == 0: ungrouped
    r, n = g(chain, 0)
    assert r.tolist() == [list(c) for c in chain] and n.tolist() == [1, 1, 1]
    assert g([], 3)[0].shape == (0, 4)


def test_person_sanity_not_parity():
    """The face of person.png is found once, where the approximate prototype found it."""
    r, n = H.group_rectangles_np(cases.person_candidates(), 3)
    assert len(r) == 1 and n[0] > 3
    x, y, w, h = (int(v) for v in r[0])
    assert w == h and 40 <= w <= 80 and abs(x + w / 2 - 390) <= 12 and abs(y + h / 2 - 89) <= 12
    r, n = H.detect_np(cases.patch(96), cases.real())
    assert len(r) == 1
    x, y, w, h = (int(v) for v in r[0])
    assert w == h and 36 <= w <= 60 and abs(x + w / 2 - 47) <= 8 and abs(y + h / 2 - 47) <= 8
    assert len(H.detect_np(np.zeros((19, 30), np.uint8), cases.real())[0]) == 0  # smaller than the window
    assert len(H.detect_np(cases.patch(96)[:20, :20], cases.real())[0]) == 0     # exactly the window


def test_defaults_are_the_references_call():
    """camera_face_demo.py:49: detectMultiScale(gray_img, scaleFactor=1.2, minNeighbors=3, minSize=(1, 1))."""
    import inspect
    assert H.DEFAULTS == dict(scale_factor=1.2, min_neighbors=3, min_size=(1, 1), max_size=None)
    sig = inspect.signature(H.CascadeClassifier.detectMultiScale).parameters
    assert [sig[k].default for k in ("scaleFactor", "minNeighbors", "minSize", "maxSize")] == [1.2, 3, (1, 1), None]
    sig = inspect.signature(H.detect_np).parameters
    assert [sig[k].default for k in ("scale_factor", "min_neighbors", "min_size", "max_size")] == [1.2, 3, (1, 1), None]


def test_crop_face_is_the_references():
    """face_demo.crop_face against what the reference's camera_face_demo.crop_face returned
    (tests/golden/haar/crop_face_ref.json, recorded by make_golden_haar.py --reference), and
    device_box against roi_crop_np."""
    demo = pkg_module("face_demo")
    roi_crop_np = pkg_module("face_detector").roi_crop_np
    ref = json.load(open(os.path.join(cases.DIR, "crop_face_ref.json")))
    frame = np.random.default_rng(ref["frame_seed"]).integers(0, 256, tuple(ref["frame"]), dtype=np.uint8)
    on_device = 0
    for case in ref["cases"]:
        padded, left_top = demo.crop_face(frame, case["rect"])
        assert list(left_top) == case["left_top"] and padded.shape == (case["side"], case["side"], 3), case
        assert hashlib.sha1(np.ascontiguousarray(padded).tobytes()).hexdigest() == case["sha1"], case
        box = demo.device_box(frame.shape, case["rect"])
        if box is not None:
            on_device += 1
            assert np.array_equal(roi_crop_np(frame, box), padded), case
        else:
            l, t = left_top
            assert not np.array_equal(roi_crop_np(frame, (l, t, l + case["side"], t + case["side"])), padded), case
    assert 4 <= on_device < len(ref["cases"])
