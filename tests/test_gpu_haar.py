"""The Haar cascade on the device (csrc/haar.hip) against its NumPy statement (haar.py), bit for bit:
every launch through op_haar_probe, the candidates and the grouped detections of a mixed batch, the
per-frame cap, staged frames read in place, and face_demo's three routes."""
import ctypes

import numpy as np
import pytest

import haar_cases as cases
from conftest import pkg_module

H = cases.haar()


@pytest.fixture(scope="module")
def real(lib):
    h = lib.HaarHandle(cases.real(), 0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def tiny(lib):
    h = lib.HaarHandle(cases.tiny(), 0)
    yield h
    h.close()


def test_last_ms_refusals(lib):
    """op_haar_last_ms as the other *_last_ms calls (host only): a null ms and a device outside
    0 .. 63 are OP_ERR_INVALID; a device no call has completed on is OP_ERR_STATE, ms untouched."""
    fn = lib.lib().op_haar_last_ms
    ms = (ctypes.c_double * 5)(*([-1.0] * 5))
    assert fn(0, None) == lib.OP_ERR_INVALID
    assert lib.last_error() == "op_haar_last_ms: null ms"
    for device in (-1, 64):
        assert fn(device, ms) == lib.OP_ERR_INVALID
        assert lib.last_error() == "op_haar_last_ms: bad device %d" % device
    assert fn(63, ms) == lib.OP_ERR_STATE
    assert lib.last_error() == ("op_haar_last_ms: no op_haar_detect or op_haar_candidates or op_haar_detect_staged or "
                                "op_haar_probe has completed on device 63")
    assert list(ms) == [-1.0] * 5


def test_null_cascade_is_refused_on_the_host(lib):
    prm = lib.haar_params()
    count, status = np.zeros(1, np.int32), np.zeros(1, np.int32)
    rc = lib.lib().op_haar_detect(None, 0, None, None, None, None, ctypes.byref(prm), 4, None, None, lib.ptr(count),
                                  lib.ptr(status))
    assert rc == lib.OP_ERR_INVALID and lib.last_error() == "op_haar_detect: null cascade"
    assert lib.lib().op_haar_destroy(None) == lib.OP_OK


def _probe_case(handle, cascade, frame, scale_factor):
    got = handle.probe(frame, scale_factor)
    maps, layers = H.result_map_np(frame, cascade, scale_factor)
    assert len(got) == len(layers) >= 5
    for i, (g, m, l) in enumerate(zip(got, maps, layers)):
        assert g["scale"] == l["scale"], i
        for k in ("pixels", "sum", "sqsum"):
            assert g[k].dtype == l[k].dtype and np.array_equal(g[k], l[k]), (i, k)
        assert np.array_equal(g["map"], m), (i, int((g["map"] != m).sum()))
    return maps


@pytest.mark.gpu
@pytest.mark.parametrize("scale_factor", [1.2, 1.1])
def test_probe_every_launch_real_cascade(real, scale_factor):
    maps = _probe_case(real, cases.real(), cases.patch(96), scale_factor)
    values = set(np.unique(np.concatenate([m.ravel() for m in maps])).tolist())
    assert {-2, 0, 1, 22} <= values and max(values) == 22  # skipped, early failures, passes


@pytest.mark.gpu
@pytest.mark.parametrize("scale_factor", [1.2, 1.1])
def test_probe_every_launch_tiny_cascade_padded_rows(tiny, scale_factor):
    frame = cases.tiny_frame(pad=3)
    assert frame.strides[0] == 64 * 3 and not frame.flags.c_contiguous
    maps = _probe_case(tiny, cases.tiny(), frame, scale_factor)
    assert set(np.unique(np.concatenate([m.ravel() for m in maps])).tolist()) == {-2, -1, 0, 1, 2}


_batch = cases.batch


def _check(rects, count, status, want, what):
    for f, w in enumerate(want):
        assert status[f] == 0 and count[f] == len(w), (what, f, count[f], len(w))
        assert np.array_equal(rects[f, :count[f]], w), (what, f)


@pytest.mark.gpu
def test_mixed_batch_equals_the_statement(lib, real):
    """One call: 96 x 96 and 64 x 64 face patches (grey), 61 x 45 noise, a constant frame, a 19 x 30 frame
    (smaller than the window), a 20 x 20 frame (exactly the window), a grey 2-D crop, and person.png at
    native size (19 scales, several chunks of every kernel's grid)."""
    frames = _batch() + [cases.person()]
    cands = list(cases.batch_candidates()) + [cases.person_candidates()]
    assert len(cands[0]) > 20 and len(cands[-1]) > 20 and not len(cands[3]) and not len(cands[4]) and not len(cands[5])
    rects, count, status = real.candidates(frames)
    _check(rects, count, status, cands, "candidates")
    rects, neigh, count, status = real.detect(frames)
    want = [H.group_rectangles_np(r, 3) for r in cands]
    _check(rects, count, status, [w[0] for w in want], "detect")
    for f, w in enumerate(want):
        assert np.array_equal(neigh[f, :count[f]], w[1]), f
    assert count[0] == 1 and count[-1] == 1
    ms = lib.haar_last_ms(0)
    assert set(ms) == set(lib.HAAR_TIMES) and ms["total"] > 0 and ms["cascade"] > 0
    assert ms["grey"] + ms["pyramid"] + ms["integrals"] + ms["cascade"] <= ms["total"] * 1.01
    assert real.detect([])[2].shape == (0,)  # n_frames == 0


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(min_neighbors=0), dict(min_neighbors=5), dict(min_size=(30, 30)), dict(max_size=(40, 40)),
                                dict(scale_factor=1.1, min_neighbors=2)],
                         ids=["neighbors0", "neighbors5", "min30", "max40", "factor1.1"])
def test_parameters_equal_the_statement(real, kw):
    frames = _batch()
    pyramid = {k: v for k, v in kw.items() if k != "min_neighbors"}
    want = [H.group_rectangles_np(r, kw.get("min_neighbors", 3)) for r in cases.batch_candidates(**pyramid)]
    rects, neigh, count, status = real.detect(frames, cap=256, **kw)
    _check(rects, count, status, [w[0] for w in want], kw)
    for f, w in enumerate(want):
        assert np.array_equal(neigh[f, :count[f]], w[1]), (kw, f)
    assert count[:2].max() >= 1  # a face is found under every one of these settings (max40: in the 64 x 64 patch only)


@pytest.mark.gpu
def test_tiny_cascade_batch_and_the_cap(lib, tiny):
    """Many survivors: a 128 x 96 noise frame overflows max_candidates=16 and reports OP_ERR_CAPACITY with
    the exact count; its neighbour is unaffected; with the cap lifted the lists are equal."""
    c = cases.tiny()
    big, small = cases.noise(96, 128, 0), cases.tiny_frame()
    want_big, want_small = H.candidates_np(big, c), H.candidates_np(small, c)
    assert len(want_big) > 2000 and 16 < len(want_small) < 4096
    rects, count, status = tiny.candidates([big, small, big], max_candidates=len(want_small), cap=len(want_small))
    assert status.tolist() == [lib.OP_ERR_CAPACITY, lib.OP_OK, lib.OP_ERR_CAPACITY]
    assert count.tolist() == [len(want_big), len(want_small), len(want_big)]
    assert np.array_equal(rects[1, :count[1]], want_small)
    few = cases.noise(9, 12, 7)
    want_few = H.candidates_np(few, c)
    assert 0 < len(want_few) <= 16
    rects, count, status = tiny.candidates([big, few, small], max_candidates=16, cap=16)
    assert status.tolist() == [lib.OP_ERR_CAPACITY, lib.OP_OK, lib.OP_ERR_CAPACITY]
    assert count.tolist() == [len(want_big), len(want_few), len(want_small)] and np.array_equal(rects[1, :count[1]], want_few)
    rects, count, status = tiny.candidates([big, small], cap=4096)
    _check(rects, count, status, [want_big, want_small], "cap lifted")
    # detect: the grouped rectangles, and a cap of rows below them
    want = H.group_rectangles_np(want_big, 3)
    rects, neigh, count, status = tiny.detect([big, small], cap=len(want[0]))
    assert status[0] == 0 and np.array_equal(rects[0, :count[0]], want[0]) and np.array_equal(neigh[0, :count[0]], want[1])
    rects, neigh, count, status = tiny.detect([big], cap=len(want[0]) - 1)
    assert status[0] == lib.OP_ERR_CAPACITY and count[0] == len(want[0])


@pytest.mark.gpu
def test_arguments_are_validated_before_any_device_call(lib, real):
    frame = cases.patch(64)
    for kw, word in ((dict(scale_factor=1.0), "scale_factor"), (dict(scale_factor=float("nan")), "scale_factor"),
                     (dict(scale_factor=float("inf")), "scale_factor"), (dict(min_size=(0, 5)), "min_size"),
                     (dict(max_size=(5, -1)), "max_size"), (dict(max_candidates=-1), "max_candidates")):
        with pytest.raises(ValueError, match=word):
            real.detect([frame], **kw)
    with pytest.raises(ValueError, match="64 scales"):
        real.detect([np.zeros((3000, 3000), np.uint8)], scale_factor=1.01)
    prm = lib.haar_params()
    hw, stride, ch = np.array([[64, 64]], np.int32), np.array([64], np.int64), np.array([1], np.int32)
    bgr = (ctypes.c_void_p * 1)(frame.ctypes.data)
    out = [np.zeros(16, np.int32), np.zeros(4, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)]

    def call(bgr=bgr, hw=hw, stride=stride, ch=ch, prm=ctypes.byref(prm), n=1):
        return lib.lib().op_haar_detect(real.h, n, bgr, lib.ptr(hw), lib.ptr(stride), lib.ptr(ch), prm, 4,
                                        *[lib.ptr(o) for o in out])
    assert call() == lib.OP_OK
    for kw, word in ((dict(hw=np.array([[64, 16385]], np.int32)), "hw"), (dict(hw=np.array([[-1, 64]], np.int32)), "hw"),
                     (dict(stride=np.array([63], np.int64)), "row_stride"), (dict(ch=np.array([2], np.int32)), "channels"),
                     (dict(bgr=None), "null bgr"), (dict(prm=None), "null params"), (dict(n=-1), "n_frames"),
                     (dict(bgr=(ctypes.c_void_p * 1)(None)), "null image")):
        assert call(**kw) == lib.OP_ERR_INVALID, kw
        assert word in lib.last_error(), (kw, lib.last_error())


@pytest.mark.gpu
def test_staged_frames_are_read_in_place(lib, ctx, real):
    render = pkg_module("render")
    frames = cases.staged_frames()
    ctx.stage_frames(frames)
    casc = H.CascadeClassifier.__new__(H.CascadeClassifier)  # the class over the module's handle
    casc._lib, casc.cascade, casc.device, casc._h = lib, cases.real(), 0, real
    want = casc.detect_batch(list(frames), with_neighbours=True)
    got = casc.detect_staged(ctx, 0, 4, with_neighbours=True)
    assert sum(len(r) for r, _ in want) >= 3
    for (r, n), (wr, wn) in zip(got, want):
        assert np.array_equal(r, wr) and np.array_equal(n, wn)
    part = casc.detect_staged(ctx, 2, 2)
    assert np.array_equal(part[0], want[2][0]) and np.array_equal(part[1], want[3][0])
    assert np.array_equal(render.render_staged(ctx, 0, 4, [[]] * 4), frames)  # the staged set is untouched
    assert np.array_equal(want[0][0], H.detect_np(frames[0], cases.real())[0])
    assert np.array_equal(casc.detectMultiScale(frames[1]), want[1][0])
    with pytest.raises(ValueError, match="outside"):
        casc.detect_staged(ctx, 3, 2)


@pytest.mark.gpu
def test_face_demo_routes_agree(lib, real, tmp_path):
    """face_demo on person.png with random FaceNet weights: the device-crop and staged routes give the
    plain route's keypoints and image (batch-invariant mode: one summation order for every forward)."""
    demo = pkg_module("face_demo")
    fd = pkg_module("face_detector").FaceDetector("facenet", model=pkg_module("weights").random_weights(2, arch="facenet"))
    fd._ctx.set_batch_invariant(True)
    casc = H.CascadeClassifier.__new__(H.CascadeClassifier)
    casc._lib, casc.cascade, casc.device, casc._h = lib, cases.real(), 0, real
    img = cases.person()
    plain = demo.run(casc, fd, [img])
    res, rects, kps = plain[0]
    assert np.array_equal(rects, H.detect_np(img, cases.real())[0]) and len(rects) == 1 and len(kps[0]) == 70
    assert demo.device_box(img.shape, rects[0]) is not None  # the device routes do cut this crop on the device
    assert res.shape == img.shape and (res != img).any()
    want = demo.annotate(img, rects, [fd(demo.crop_face(img, rects[0])[0])])
    assert np.array_equal(res, want)
    for kw in (dict(device_crops=True), dict(staged=True)):
        other = demo.run(casc, fd, [img], **kw)[0]
        assert np.array_equal(other[1], rects) and other[2] == kps and np.array_equal(other[0], res), kw
    # the CLI (seeded random weights, other than the ones above: a plumbing run)
    from PIL import Image
    src, dst = str(tmp_path / "person.png"), tmp_path / "faces.png"
    Image.fromarray(np.ascontiguousarray(img[:, :, ::-1])).save(src)
    assert demo.main(["--cascade", cases.REAL_XML, "--random-weights", "--img", src, "--out", str(dst), "--device-crops"]) == 0
    back = np.asarray(Image.open(str(dst)).convert("RGB"))[:, :, ::-1]
    assert back.shape == img.shape and (back != img).any()
    assert (back[59, 360:421] == 255).all(axis=1).mean() > 0.5  # the rectangle's top edge (keypoints may cross it)
