"""ROI detection on the GPU (op_cpm_detect_rois): the detector fed with frames and integer boxes
cuts, mirrors and resizes the crops on the device and post-processes every ROI of a group in a
fixed number of launches.  Held bit for bit to the path it replaces: detect_batch on the crops
roi_crop_np states (the host crop, and the host flip of a left hand)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden, people_image, pkg_module

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctxs():
    """arch -> (CpmContext, weights), made on first use (random weights, seed 4)."""
    lib = pkg_module("_lib")
    made = {}

    def get(arch):
        if arch not in made:
            c = lib.CpmContext(arch, 0)
            c.set_weights(pkg_module("weights").random_weights(seed=4, arch=arch))
            made[arch] = c
        return made[arch]

    yield get
    for c in made.values():
        c.close()


@pytest.fixture(scope="module", params=["facenet", "handnet"])
def cpm(request, ctxs):
    return request.param, ctxs(request.param)


def _same(got, exp):
    assert len(got) == len(exp)
    for i, (g, e) in enumerate(zip(got, exp)):
        assert (g is None) == (e is None), i
        if g is not None:
            assert g[0] == e[0] and g[1] == e[1] and np.float32(g[2]) == np.float32(e[2]), (i, g, e)


def _same_all(got, exp):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        _same(g, e)


_rng = np.random.default_rng(21)
FRAME_A = _rng.integers(0, 256, (97, 131, 3), dtype=np.uint8)
FRAME_B = _rng.integers(0, 256, (80, 100, 3), dtype=np.uint8)[7:57, 11:75]  # 50 x 64, rows 300 B apart
FRAMES = [FRAME_A, FRAME_B]
FRAME_BYTES = 97 * 131 * 3 + 50 * 64 * 3
# (frame, (left, top, right, bottom))
BOXES = [(0, (10, 12, 71, 90)),        # inside, odd-sized
         (0, (-7, -5, 40, 33)),        # across left / top
         (1, (-7, -5, 40, 33)),
         (0, (100, 60, 150, 120)),     # across right / bottom
         (1, (-9, -6, 75, 61)),        # larger than the frame on every side
         (0, (200, 200, 240, 230)),    # wholly outside: an all-zero crop
         (1, (0, 0, 2, 2)),            # the smallest box
         (0, (0, 0, 131, 97)),         # the full frames
         (1, (0, 0, 64, 50))]


def _rois(arch):
    """(frame ids, boxes, mirror flags): every handnet ROI once unmirrored and once mirrored."""
    rois = [(f, b, False) for f, b in BOXES]
    if arch == "handnet":
        rois = [(f, b, m) for f, b in BOXES for m in (False, True)]
    return [r[0] for r in rois], [r[1] for r in rois], [r[2] for r in rois]


_expected = {}


def _host_path(arch, c, thr, invariant):
    """The path detect_rois replaces, once per (arch, mode, threshold): detect_batch on host crops."""
    key = (arch, bool(invariant), float(thr))
    if key not in _expected:
        roi_crop_np = pkg_module("face_detector").roi_crop_np
        fids, boxes, mirror = _rois(arch)
        crops = [roi_crop_np(FRAMES[f], b, m) for f, b, m in zip(fids, boxes, mirror)]
        _expected[key] = c.detect_batch(crops, thr, flip_maps=mirror)
    return _expected[key]


@pytest.mark.parametrize("invariant", [False, True])
def test_detect_rois_equals_detect_batch_on_host_crops(cpm, invariant):
    arch, c = cpm
    assert FRAME_B.strides[0] == 300 and not FRAME_B.flags.c_contiguous
    fids, boxes, mirror = _rois(arch)
    c.set_batch_invariant(invariant)
    try:
        thresholds = [-10.0, 0.05]
        n_found = 0
        for thr in thresholds:
            exp = _host_path(arch, c, thr, invariant)
            got = c.detect_rois(FRAMES, boxes, thr, frame_ids=fids, mirror=mirror)
            _same_all(got, exp)
            if thr == -10.0:
                assert all(k is not None for kps in exp for k in kps)
                if not any(k is not None for kps in _host_path(arch, c, 0.05, invariant) for k in kps):
                    # a threshold the random-weight maps cross, so keypoints are found and missed
                    thresholds.append(float(np.float32(np.median([k[2] for kps in exp for k in kps]))))
            else:
                n_found = max(n_found, sum(k is not None for kps in exp for k in kps))
        print("%s invariant=%d thresholds %s: %d keypoints found" % (arch, invariant, thresholds, n_found))
        assert n_found > 0
        # one frame given bare, default frame ids and mirror flags; a smaller batch, so the same
        # bits only where a ROI's sums do not depend on its batch
        one = c.detect_rois(FRAME_A, [b for f, b in BOXES if f == 0], 0.05)
        pick = [i for i, (f, m) in enumerate(zip(fids, mirror)) if f == 0 and not m]
        assert len(one) == len(pick)
        if invariant:
            _same_all(one, [_host_path(arch, c, 0.05, invariant)[i] for i in pick])
    finally:
        c.set_batch_invariant(False)


def test_detect_rois_downscaling_box(ctxs):
    """A box larger than the network input on both sides: the decimating side of the resize."""
    c = ctxs("handnet")
    roi_crop_np = pkg_module("face_detector").roi_crop_np
    frame = np.random.default_rng(22).integers(0, 256, (400, 420, 3), dtype=np.uint8)
    box = (0, 0, 400, 390)
    for thr in (-10.0, 0.05):
        for m in (False, True):
            _same_all(c.detect_rois(frame, [box], thr, mirror=[m]),
                      c.detect_batch([roi_crop_np(frame, box, m)], thr, flip_maps=[m]))


def test_detect_rois_groups(cpm):
    arch, c = cpm
    lib = pkg_module("_lib")
    k = lib.CpmContext.ROI_GROUP_LAUNCHES
    assert 1 <= k <= 4
    fids, boxes, mirror = _rois(arch)
    n = len(boxes)
    exp = _host_path(arch, c, 0.05, False)
    one = c.detect_rois(FRAMES, boxes, 0.05, frame_ids=fids, mirror=mirror)
    s1 = c.roi_stats()
    c.set_roi_group_bytes(1 << 20)
    try:
        many = c.detect_rois(FRAMES, boxes, 0.05, frame_ids=fids, mirror=mirror)
        sm = c.roi_stats()
    finally:
        c.set_roi_group_bytes(0)
    print(arch, "default", s1, "1 MiB groups", sm)
    assert s1["groups"] == 1 and sm["groups"] >= 3
    _same_all(one, exp)
    _same_all(many, exp)
    for s in (s1, sm):
        assert s["launches"] == 1 + k * s["groups"]
        assert s["upload_bytes"] == FRAME_BYTES + lib.CpmContext.roi_table_bytes(2, n)
    assert sm["scratch_bytes"] < s1["scratch_bytes"]
    # twice the ROIs on the same frames: the same launches, the same frame bytes
    two = c.detect_rois(FRAMES, boxes + boxes, 0.05, frame_ids=fids + fids, mirror=mirror + mirror)
    s2 = c.roi_stats()
    assert s2["groups"] == 1 and s2["launches"] == s1["launches"] == 1 + k
    assert s2["upload_bytes"] == FRAME_BYTES + lib.CpmContext.roi_table_bytes(2, 2 * n)
    assert len(two) == 2 * n


def test_detect_rois_errors(cpm):
    arch, c = cpm
    fids, boxes, mirror = _rois(arch)
    exp = _host_path(arch, c, 0.05, False)
    with pytest.raises(ValueError, match="ROI 1"):
        c.detect_rois(FRAMES, [boxes[0], (5, 5, 6, 40), boxes[2]], 0.05)
    with pytest.raises(ValueError, match="ROI 2"):
        c.detect_rois(FRAMES, boxes[:3], 0.05, frame_ids=[0, 1, 2])
    with pytest.raises(ValueError, match="ROI 0"):
        c.detect_rois(FRAMES, [(0, 0, 2 ** 30 + 1, 2)], 0.05)
    with pytest.raises(ValueError, match="ROI 0"):
        c.detect_rois(FRAMES, [(0, 0, 2 ** 16, 2 ** 15)], 0.05)  # an area of 2^31
    with pytest.raises(ValueError):
        c.detect_rois(FRAMES, boxes[:2], 0.05, frame_ids=[0])
    assert c.detect_rois(FRAMES, [], 0.05) == []
    # a failed call leaves the context as it was
    _same_all(c.detect_rois(FRAMES, boxes, 0.05, frame_ids=fids, mirror=mirror), exp)
    bare = pkg_module("_lib").CpmContext(arch, 0)
    try:
        with pytest.raises(RuntimeError, match="weights"):
            bare.detect_rois(FRAMES, boxes[:1], 0.05)
    finally:
        bare.close()


def test_demo_run_device_crops(tmp_path):
    """demo.run on people.png with the six-person golden poses standing in for the pose detector:
    device_crops draws the default path's image, with and without device_draw."""
    demo = pkg_module("demo")
    W = pkg_module("weights")
    pd = pkg_module("pose_detector").PoseDetector("posenet", model=W.random_weights(0))
    poses = load_golden("six_people")["poses"]

    class Pose(object):
        def __call__(self, img):
            return poses.copy(), np.ones(len(poses))

        def __getattr__(self, name):
            return getattr(pd, name)

    fd = pkg_module("face_detector").FaceDetector("facenet", model=W.random_weights(2, arch="facenet"))
    hd = pkg_module("hand_detector").HandDetector("handnet", model=W.random_weights(2, arch="handnet"))
    img = people_image()
    quiet = lambda s: None
    want = demo.run(img, Pose(), fd, hd, log=quiet)
    got = demo.run(img, Pose(), fd, hd, log=quiet, device_crops=True)
    assert (want != img).any() and np.array_equal(got, want)
    assert fd._ctx.roi_stats()["groups"] >= 1 and hd._ctx.roi_stats()["upload_bytes"] > img.size
    want_dd = demo.run(img, Pose(), fd, hd, log=quiet, device_draw=True)
    got_dd = demo.run(img, Pose(), fd, hd, log=quiet, device_draw=True, device_crops=True)
    assert np.array_equal(got_dd, want_dd)
    dst = tmp_path / "result.png"
    src = os.path.join(GOLDEN, "people.png")
    assert demo.main(["--img", src, "--random-weights", "--device-crops", "--out", str(dst)]) == 0 and dst.exists()
