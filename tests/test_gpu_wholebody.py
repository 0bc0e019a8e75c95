"""Whole-body detection over a staged batch on the GPU: the boxes made on the device from poses
(op_body_rois / op_body_rois_staged, csrc/body.hip) held bit for bit to ``wholebody.body_rois_np``,
FaceNet / HandNet on staged frames read in place (op_cpm_detect_rois_staged) held bit for bit to
``detect_rois`` on the same frames given from the host, the chunked forwards, the argument checks,
and ``wholebody.detect_staged`` / ``demo.run_batch`` end to end against the chain made by hand."""
import ctypes

import numpy as np
import pytest

import wholebody_cases as cases
from conftest import load_golden, pkg_module

pytestmark = pytest.mark.gpu

H = W = 480  # the network input is 368 x 368: the 46 x 46 maps of six_people fit
FRAMES = np.random.default_rng(31).integers(0, 256, (2, H, W, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def wb():
    return pkg_module("wholebody")


@pytest.fixture(scope="module")
def pd(rand_weights):
    """A PoseDetector whose staged step post-processes staged maps: the six_people maps for frame 0
    and all-zero maps for frame 1 (7 persons, then none)."""
    det = pkg_module("pose_detector").PoseDetector("posenet", model=rand_weights, max_batch=2)
    d = load_golden("six_people")
    maps = np.zeros((2, 57, 46, 46), np.float32)
    maps[0] = np.concatenate([d["paf_low"], d["heat_low"]])
    ctx = det.staged_context()
    ctx.stage_frames(FRAMES)
    ctx.stage_maps(maps)
    ctx.use_staged_maps(True)
    ctx.run_staged()
    ctx.synchronize()
    yield det
    ctx.use_staged_maps(False)


@pytest.fixture(scope="module")
def staged(pd, wb):
    """The staged step's results, fetched once, and the statement's boxes of them."""
    ctx = pd.staged_context()
    results = ctx.fetch_results(0, 2)
    poses = results[0][0]
    assert len(poses) == 7 and len(results[1][0]) == 0
    unit, box, state = wb.body_rois_np(poses)
    faces = [(0, tuple(int(v) for v in box[p, 0])) for p in range(7) if state[p, 0] == wb.VALID]
    hands = [(0, tuple(int(v) for v in box[p, k]), side) for p in range(7) for k, side in ((1, "left"), (2, "right"))
             if state[p, k] == wb.VALID]
    assert len(faces) == 5 and len(hands) == 12 and sum(h[2] == "left" for h in hands) == 6
    assert (state != wb.SKIPPED).all()
    return {"ctx": ctx, "results": results, "poses": poses, "unit": unit, "box": box, "state": state,
            "faces": faces, "hands": hands}


@pytest.fixture(scope="module")
def fd():
    W_ = pkg_module("weights")
    return pkg_module("face_detector").FaceDetector("facenet", model=W_.random_weights(seed=4, arch="facenet"))


@pytest.fixture(scope="module")
def hd():
    W_ = pkg_module("weights")
    return pkg_module("hand_detector").HandDetector("handnet", model=W_.random_weights(seed=4, arch="handnet"))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_all(got, exp):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        assert len(g) == len(e)
        for a, b in zip(g, e):
            assert (a is None) == (b is None)
            if a is not None:
                assert a[0] == b[0] and a[1] == b[1] and np.float32(a[2]) == np.float32(b[2]), (a, b)


def test_body_rois_bit_identical_to_the_statement(lib, wb):
    synth, names = cases.synthetic()
    poses = np.concatenate([synth, cases.fixture_poses()])
    before = poses.copy()
    unit, box, state = lib.body_rois(poses)
    w_unit, w_box, w_state = wb.body_rois_np(before)
    assert np.array_equal(_bits(poses), _bits(before))
    bad = [names[i] if i < len(names) else "fixture %d" % (i - len(names)) for i in range(len(poses))
           if _bits(unit)[i] != _bits(w_unit)[i] or not np.array_equal(box[i], w_box[i])
           or not np.array_equal(state[i], w_state[i])]
    print("%d persons, states %s, kernel + upload %.3f ms" % (len(poses), np.bincount(state.ravel(), minlength=3),
                                                             lib.body_last_ms(0)))
    assert not bad, bad
    assert set(np.unique(state)) == {wb.ABSENT, wb.VALID, wb.SKIPPED}
    assert lib.body_rois(np.zeros((0, 18, 3)))[0].shape == (0,)


def test_body_rois_staged(lib, wb, staged):
    ctx = staged["ctx"]
    raw_before = [(p.tobytes(), s.tobytes()) for p, s, _ in ctx.fetch_results(0, 2)]
    count, status, unit, box, state = ctx.body_rois(0, 2, cap=8)
    assert list(count) == [7, 0] and list(status) == [lib.OP_OK, lib.OP_OK]
    assert np.array_equal(_bits(unit[0, :7]), _bits(staged["unit"]))
    assert np.array_equal(box[0, :7], staged["box"]) and np.array_equal(state[0, :7], staged["state"])
    assert not unit[0, 7:].any() and not box[0, 7:].any() and not state[0, 7:].any()
    assert not unit[1].any() and not box[1].any() and not state[1].any()
    # frame 1 alone, and a cap below the persons found: OP_ERR_CAPACITY naming the rows needed
    c1 = ctx.body_rois(1, 1, cap=3)
    assert list(c1[0]) == [0] and not c1[4].any()
    cap = 4
    cnt, st = np.zeros(2, np.int32), np.zeros(2, np.int32)
    u, b, s = np.zeros((2, cap)), np.zeros((2, cap, 3, 4), np.int32), np.zeros((2, cap, 3), np.int32)
    rc = lib.lib().op_body_rois_staged(ctx.h, 0, 2, cap, lib.ptr(cnt), lib.ptr(st), lib.ptr(u), lib.ptr(b), lib.ptr(s))
    assert rc == lib.OP_ERR_CAPACITY and "7 rows" in lib.last_error() and list(cnt) == [7, 0]
    assert np.array_equal(_bits(u[0]), _bits(staged["unit"][:cap])) and np.array_equal(b[0], staged["box"][:cap])
    # the result rows were only read
    raw_after = [(p.tobytes(), s.tobytes()) for p, s, _ in ctx.fetch_results(0, 2)]
    assert raw_after == raw_before
    for args in ((2, 1, 8), (-1, 1, 8), (0, 3, 8), (0, 0, 8), (0, 2, 0)):
        with pytest.raises(ValueError):
            ctx.body_rois(*args)


def _rois(staged, arch):
    if arch == "facenet":
        return [f[1] for f in staged["faces"]], [f[0] for f in staged["faces"]], None
    return ([h[1] for h in staged["hands"]], [h[0] for h in staged["hands"]],
            [h[2] == "left" for h in staged["hands"]])


@pytest.mark.parametrize("arch", ["facenet", "handnet"])
def test_detect_rois_staged_equals_detect_rois(lib, staged, fd, hd, arch):
    c = (fd if arch == "facenet" else hd)._ctx
    boxes, fids, mirror = _rois(staged, arch)
    n = len(boxes)
    for thr in (-10.0, 0.05):
        exp = c.detect_rois(list(FRAMES), boxes, thr, frame_ids=fids, mirror=mirror)
        host_bytes = c.roi_stats()["upload_bytes"]
        got = c.detect_rois_staged(staged["ctx"], 0, 2, boxes, thr, frame_ids=fids, mirror=mirror)
        stats = c.roi_stats()
        _same_all(got, exp)
        if thr < 0:
            assert all(k is not None for kps in got for k in kps)
        assert stats["upload_bytes"] == 24 * 2 + 48 * n == lib.CpmContext.roi_table_bytes(2, n)
        assert host_bytes == FRAMES.size + stats["upload_bytes"]
        assert stats["launches"] == 1 + lib.CpmContext.ROI_GROUP_LAUNCHES * stats["groups"]
    # a sub-range of the staged set: frame 1 alone is staged frame `first` = 1
    one = [(3, 5, 60, 70), (-4, 400, 90, 500)]
    _same_all(c.detect_rois_staged(staged["ctx"], 1, 1, one, -10.0),
              c.detect_rois(FRAMES[1], one, -10.0))
    assert c.detect_rois_staged(staged["ctx"], 0, 2, [], 0.05) == []


def test_detect_rois_staged_chunks(lib, staged, hd):
    c = hd._ctx
    boxes, fids, mirror = _rois(staged, "handnet")
    n = len(boxes)
    assert n == 12
    c.set_batch_invariant(True)
    try:
        host = c.detect_rois(list(FRAMES), boxes, -10.0, frame_ids=fids, mirror=mirror)
        whole = c.detect_rois_staged(staged["ctx"], 0, 2, boxes, -10.0, frame_ids=fids, mirror=mirror)
        s0 = c.roi_stats()
        c.set_roi_batch(5)  # chunks of 5, 5 and 2
        parts = c.detect_rois_staged(staged["ctx"], 0, 2, boxes, -10.0, frame_ids=fids, mirror=mirror)
        s5 = c.roi_stats()
        c.set_roi_batch(0)
        _same_all(whole, host)
        _same_all(parts, whole)
        assert s0["upload_bytes"] == 24 * 2 + 48 * n and s5["upload_bytes"] == 3 * 24 * 2 + 48 * n
        assert s5["groups"] == 3 and s5["launches"] == 3 * (1 + lib.CpmContext.ROI_GROUP_LAUNCHES)
        assert s5["scratch_bytes"] < s0["scratch_bytes"]
        # the existing entry is as it was
        _same_all(c.detect_rois(list(FRAMES), boxes, -10.0, frame_ids=fids, mirror=mirror), host)
        with pytest.raises(ValueError):
            c.set_roi_batch(-1)
    finally:
        c.set_roi_batch(0)
        c.set_batch_invariant(False)


def test_detect_rois_staged_argument_errors(lib, staged, hd):
    """Every case is refused on the host (OP_ERR_INVALID -> ValueError) before anything is launched."""
    c = hd._ctx
    ctx = staged["ctx"]
    good = [(10, 10, 60, 70)]
    empty = lib.Context(0)
    try:
        with pytest.raises(ValueError, match="no staged frames"):
            c.detect_rois_staged(empty, 0, 1, good, 0.05)
    finally:
        empty.close()
    before = c.roi_stats()
    for first, n_frames in ((1, 2), (2, 1), (-1, 1), (0, 0), (0, 3)):
        with pytest.raises(ValueError, match="staged frames"):
            c.detect_rois_staged(ctx, first, n_frames, good, 0.05)
    with pytest.raises(ValueError, match="ROI 1"):
        c.detect_rois_staged(ctx, 0, 2, good * 2, 0.05, frame_ids=[1, 2])
    with pytest.raises(ValueError, match="ROI 0"):
        c.detect_rois_staged(ctx, 0, 2, good, 0.05, frame_ids=[-1])
    with pytest.raises(ValueError, match="ROI 2"):
        c.detect_rois_staged(ctx, 0, 2, good * 2 + [(5, 5, 6, 40)], 0.05)  # r - l < 2
    c.set_roi_batch(2)
    try:
        with pytest.raises(ValueError, match="ROI 4"):  # in the third chunk: still before the first launch
            c.detect_rois_staged(ctx, 0, 2, good * 4 + [(5, 5, 40, 6)], 0.05)
    finally:
        c.set_roi_batch(0)
    with pytest.raises(ValueError):
        c.detect_rois_staged(ctx, 0, 2, good * 2, 0.05, frame_ids=[0])
    rc = lib.lib().op_cpm_detect_rois_staged(c.h, None, 0, 1, 1, None, None, None, ctypes.c_float(0.05), None, None)
    assert rc == lib.OP_ERR_INVALID
    assert c.roi_stats() == before  # nothing ran
    bare = lib.CpmContext("handnet", 0)
    try:
        with pytest.raises(RuntimeError, match="weights"):
            bare.detect_rois_staged(ctx, 0, 2, good, 0.05)
    finally:
        bare.close()


def _chain(pd, fd, hd, results):
    """demo.run's device_crops chain by hand, per frame: fetch_results' poses, the host helpers,
    detect_rois on the host frames -> [(poses, face items, hand items)]."""
    out = []
    for i, (poses, scores, _) in enumerate(results):
        faces, hands = [], []
        for pose in poses:
            pose = pose.copy()
            u = pd.get_unit_length(pose)
            faces.append(pd.face_bbox(pose, u))
            hands.append(pd.hand_bboxes(pose, u))
        fb = [b for b in faces if b is not None]
        hb = [(h[side], side) for h in hands for side in ("left", "right") if h[side] is not None]
        fk = iter(fd.detect_rois(FRAMES[i], fb) if fb else [])
        hk = iter(hd.detect_rois(FRAMES[i], [b for b, _ in hb], [s for _, s in hb]) if hb else [])
        face_items = [None if b is None else (next(fk), b) for b in faces]
        hand_items = [{side: None if h[side] is None else (next(hk), h[side]) for side in ("left", "right")} for h in hands]
        out.append((poses, scores, face_items, hand_items))
    return out


def test_detect_staged_and_run_batch_end_to_end(lib, wb, pd, fd, hd, staged):
    render = pkg_module("render")
    demo = pkg_module("demo")
    # one forward per network in both paths (7 persons in one frame), so the same bits without
    # the batch-invariant mode only if the batches agree: they do, frame 1 adds no ROI
    chain = _chain(pd, fd, hd, staged["results"])
    got = wb.detect_staged(pd, fd, hd, 0, 2)
    assert [len(f) for f in got] == [7, 0]
    assert fd._ctx.roi_stats()["upload_bytes"] == 24 * 2 + 48 * 5
    assert hd._ctx.roi_stats()["upload_bytes"] == 24 * 2 + 48 * 12
    for persons, (poses, scores, face_items, hand_items) in zip(got, chain):
        for p, person in enumerate(persons):
            assert np.array_equal(person["pose"], poses[p]) and person["score"] == scores[p]
            assert _bits([person["unit"]])[0] == _bits(staged["unit"])[p] and person["skipped"] == ()
            for item, want in ((person["face"], face_items[p]), (person["hands"]["left"], hand_items[p]["left"]),
                               (person["hands"]["right"], hand_items[p]["right"])):
                assert (item is None) == (want is None)
                if item is not None:
                    assert tuple(item[1]) == tuple(want[1])
                    _same_all([item[0]], [want[0]])
    want_imgs = render.render(list(FRAMES), [render.demo_list(poses, f, h) for poses, _, f, h in chain])
    imgs = demo.run_batch(list(FRAMES), pd, fd, hd, log=lambda s: None)
    assert len(imgs) == 2
    for a, b, src in zip(imgs, want_imgs, FRAMES):
        assert np.array_equal(a, b)
    assert (imgs[0] != FRAMES[0]).any() and np.array_equal(imgs[1], render.render_np(FRAMES[1], [render.DEMO_BLEND]))
    host = demo.run_batch(list(FRAMES), pd, fd, hd, log=lambda s: None, device_draw=False)
    assert np.array_equal(host[0], imgs[0]) and np.array_equal(host[1], imgs[1])
