"""wholebody.py on the host: ``body_rois_np`` (the statement the device kernel is held to in
test_gpu_wholebody.py) against the helpers it restates, its branches on synthetic persons, and the
ROI ordering and fallback merging of ``detect_staged`` with the device calls replaced."""
import numpy as np
import pytest

import wholebody_cases as cases
from conftest import pkg_module


@pytest.fixture(scope="module")
def wb():
    return pkg_module("wholebody")


@pytest.fixture(scope="module")
def helpers():
    """A PoseDetector that was never constructed: the box helpers need no device."""
    PoseDetector = pkg_module("pose_detector").PoseDetector
    return object.__new__(PoseDetector)


def _runnable(b):
    return (all(abs(v) <= 2 ** 30 for v in b) and b[2] - b[0] >= 2 and b[3] - b[1] >= 2
            and (b[2] - b[0]) * (b[3] - b[1]) < 2 ** 31)


def test_pairwise_sum_is_np_sum(wb):
    rng = np.random.default_rng(3)
    for n in range(20):
        for _ in range(200):
            x = rng.uniform(0.0, 500.0, n) / rng.choice([0.2, 0.85, 2.2, 0.93], n)
            assert wb.pairwise_sum(x) == np.sum(x), n


def test_body_rois_np_equals_the_helpers_on_the_fixtures(wb, helpers):
    poses = cases.fixture_poses()
    assert poses.shape == (31, 18, 3)
    before = poses.copy()
    unit, box, state = wb.body_rois_np(poses)
    assert np.array_equal(poses, before)  # the shift of the hands stays local
    assert unit.dtype == np.float64 and box.dtype == np.int32 and state.dtype == np.int32
    seen = {"no_nose": 0, "no_hands": 0, "outside": 0, "three_joints": 0}
    for p, pose in enumerate(before):
        u = helpers.get_unit_length(pose.copy())
        assert np.isclose(unit[p], u, rtol=1e-12, atol=0.0), (p, unit[p], u)
        face = helpers.face_bbox(pose.copy(), u)
        hands = helpers.hand_bboxes(pose.copy(), u)
        for k, want in enumerate((face, hands["left"], hands["right"])):
            assert (state[p, k] != wb.ABSENT) == (want is not None), (p, k)
            if want is None:
                assert not box[p, k].any()
            elif state[p, k] == wb.VALID:
                assert tuple(int(v) for v in box[p, k]) == tuple(want), (p, k)
                seen["outside"] += min(want) < 0
            else:
                assert state[p, k] == wb.SKIPPED and not _runnable(want) and not box[p, k].any(), (p, k, want)
        seen["no_nose"] += face is None
        seen["no_hands"] += hands["left"] is None and hands["right"] is None
        seen["three_joints"] += int((pose[:, 2] > 0).sum()) == 3
    assert all(v > 0 for v in seen.values()), seen


def test_body_rois_np_branches(wb):
    poses, names = cases.synthetic()
    unit, box, state = wb.body_rois_np(poses)
    at = {n: i for i, n in enumerate(names)}
    L = cases.limbs()

    def terms(p, idx, div):
        out = []
        for i, d in zip(idx, div):
            a, b = L[i]
            v = np.sqrt((p[b][0] - p[a][0]) ** 2 + (p[b][1] - p[a][1]) ** 2)
            if v > 0:
                out.append(v / d)
        return out

    for want in (14, 9, 8, 7):  # the fallback: np.sum over that many terms
        i = at["fallback_%d_found" % want]
        t = terms(poses[i], range(19), wb.UNIT_ALL_DIV)
        assert len(t) == want and unit[i] == np.sum(np.array(t)) / want
    for want in (19, 17, 16):
        i = at["base_%d_found" % want]
        t = terms(poses[i], wb.UNIT_BASE, wb.UNIT_BASE_DIV)
        assert len(t) == 5 and unit[i] == np.sum(np.array(t)) / 5
    i = at["left_elbow_absent_no_shift"]
    s = unit[i] * 0.95
    x, y = poses[i][cases.L_HAND][:2]
    assert state[i, 1] == wb.VALID and tuple(box[i, 1]) == (int(x - s), int(y - s), int(x + s), int(y + s))
    i = at["right_hand_on_its_elbow"]
    s = unit[i] * 0.95
    x, y = poses[i][cases.R_HAND][:2]
    assert state[i, 2] == wb.VALID and tuple(box[i, 2]) == (int(x - s), int(y - s), int(x + s), int(y + s))
    i = at["unit_below_one_pixel_state_2"]
    assert 0 < unit[i] < 0.5 and (state[i] == wb.SKIPPED).all() and not box[i].any()
    i = at["nan_left_hand_state_2"]
    assert np.isfinite(unit[i]) and list(state[i]) == [wb.VALID, wb.SKIPPED, wb.VALID] and not box[i, 1].any()
    i = at["nan_nose_state_2"]
    assert np.isfinite(unit[i]) and list(state[i]) == [wb.SKIPPED, wb.VALID, wb.VALID]
    i = at["1e12_right_hand_state_2"]
    assert np.isfinite(unit[i]) and list(state[i]) == [wb.VALID, wb.VALID, wb.SKIPPED]
    i = at["inf_nose_unit_not_finite"]
    assert not np.isfinite(unit[i]) and (state[i] == wb.SKIPPED).all()
    i = at["negative_coordinates_trunc_is_not_floor"]
    nx, ny = poses[i][cases.NOSE][:2]
    u = unit[i]
    exact = np.array([nx - u, ny - u * 1.2, nx + u, ny + u * 0.8])
    assert state[i, 0] == wb.VALID and (box[i, 0] == np.trunc(exact)).all() and (box[i, 0] != np.floor(exact)).any()
    i = at["one_point_no_limb_unit_nan"]
    assert unit[i:i + 1].view(np.uint64)[0] == 0x7FF8000000000000 and (state[i] == wb.SKIPPED).all()
    i = at["no_nose_no_hands"]
    assert (state[i] == wb.ABSENT).all() and not box[i].any() and unit[i] > 0
    i = at["three_joints"]
    assert (state[i] == wb.ABSENT).all() and unit[i] > 0
    assert wb.body_rois_np(np.zeros((0, 18, 3)))[1].shape == (0, 3, 4)


class _FakeCtx(object):
    """Stands where the pose context does: ``frames`` {staged index: poses}; the frames of
    ``over_caps`` report OP_ERR_CAPACITY and count 0, as a frame over the batched caps does."""

    def __init__(self, wb, lib, frames, over_caps):
        self.wb, self.lib, self.frames, self.over_caps = wb, lib, frames, over_caps
        self.calls = []

    def body_rois(self, first, n, cap):
        self.calls.append(("body_rois", first, n, cap))
        count = np.zeros(n, np.int32)
        status = np.zeros(n, np.int32)
        unit = np.zeros((n, cap))
        box = np.zeros((n, cap, 3, 4), np.int32)
        state = np.zeros((n, cap, 3), np.int32)
        for i in range(n):
            poses = self.frames[first + i]
            if first + i in self.over_caps:
                status[i] = self.lib.OP_ERR_CAPACITY
                continue
            count[i] = len(poses)
            k = min(len(poses), cap)
            unit[i, :k], box[i, :k], state[i, :k] = self.wb.body_rois_np(poses[:k])
        return count, status, unit, box, state

    def fetch_results(self, first, n, cap=64):
        self.calls.append(("fetch_results", first, n))
        return [self.fetch_result(first + i)[:3] for i in range(n)]

    def fetch_result(self, frame, cap=2048):
        self.calls.append(("fetch_result", frame))
        return self.frames[frame].copy(), np.arange(len(self.frames[frame])) + 0.5, None


class _FakePose(object):
    device = 0

    def __init__(self, ctx):
        self.ctx = ctx

    def staged_context(self):
        return self.ctx


class _FakeCpm(object):
    def __init__(self, hand):
        self.hand, self.calls, self.batch = hand, [], None

    def set_roi_batch(self, rois):
        self.batch = rois

    def detect_rois_staged(self, ctx, first, n_frames, bboxes, *rest):
        types, frame_ids = (rest[0], rest[1]) if self.hand else (None, rest[0])
        self.calls.append((first, n_frames, list(bboxes), list(frame_ids), types))
        return [["kp", i] for i in range(len(bboxes))]


def test_detect_staged_roi_order_and_fallback(wb, lib, monkeypatch):
    six = cases.fixture_poses()[:7]
    synth, names = cases.synthetic()
    skip = synth[names.index("nan_left_hand_state_2")]
    # frame 6 is over the batched caps, frame 7 has more persons than cap
    ctx_frames = {5: np.concatenate([six[:2], skip[None]]), 6: six[2:4], 7: six[:7]}
    cap = 4
    ctx = _FakeCtx(wb, lib, ctx_frames, {6})
    device_calls = []
    monkeypatch.setattr(lib, "body_rois", lambda poses, device=0: device_calls.append(len(poses)) or wb.body_rois_np(poses))
    fd, hd = _FakeCpm(False), _FakeCpm(True)
    out = wb.detect_staged(_FakePose(ctx), fd, hd, 5, 3, roi_batch=9, cap=cap)
    top = [c for c in ctx.calls if c[0] != "fetch_result"]
    assert top == [("body_rois", 5, 3, cap), ("fetch_results", 5, 3)]
    assert [c[1] for c in ctx.calls if c[0] == "fetch_result"][3:] == [6, 7] and device_calls == [2, 7]
    assert fd.batch == 9 and hd.batch == 9 and len(fd.calls) == 1 and len(hd.calls) == 1
    assert [len(f) for f in out] == [3, 2, 7]
    # the expected ROI lists, in demo.run's order, from the statement
    want_face, want_hand = [], []
    for i, k in enumerate((5, 6, 7)):
        unit, box, state = wb.body_rois_np(ctx_frames[k])
        for p in range(len(unit)):
            person = out[i][p]
            assert np.array_equal(person["pose"], ctx_frames[k][p], equal_nan=True) and person["score"] == p + 0.5
            assert person["unit"] == unit[p] or (np.isnan(unit[p]) and np.isnan(person["unit"]))
            if state[p, 0] == wb.VALID:
                want_face.append((i, tuple(box[p, 0])))
            for j, side in ((1, "left"), (2, "right")):
                if state[p, j] == wb.VALID:
                    want_hand.append((i, tuple(box[p, j]), side))
    first, n_frames, bboxes, fids, types = fd.calls[0]
    assert (first, n_frames, types) == (5, 3, None) and list(zip(fids, bboxes)) == want_face and len(want_face) >= 5
    first, n_frames, bboxes, fids, types = hd.calls[0]
    assert (first, n_frames) == (5, 3) and list(zip(fids, bboxes, types)) == want_hand
    assert {"left", "right"} <= set(types) and {0, 1, 2} <= set(fids)
    # the keypoints went back to their persons in the same order
    nf = nh = 0
    for persons in out:
        for person in persons:
            if person["face"] is not None and person["face"][0] is not None:
                assert person["face"] == (["kp", nf], want_face[nf][1])
                nf += 1
            for side in ("left", "right"):
                item = person["hands"][side]
                if item is not None and item[0] is not None:
                    assert item == (["kp", nh], want_hand[nh][1])
                    nh += 1
    assert nf == len(want_face) and nh == len(want_hand)
    skipped = out[0][2]
    assert skipped["skipped"] == ("left",) and skipped["hands"]["left"] == (None, None) and skipped["face"][0] is not None
    assert all(p["skipped"] == () for f in out for p in f if p is not skipped)


def test_detect_staged_without_persons(wb, lib):
    class Ctx(object):
        def body_rois(self, first, n, cap):
            return (np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, cap)), np.zeros((n, cap, 3, 4), np.int32),
                    np.zeros((n, cap, 3), np.int32))

        def fetch_results(self, first, n, cap=64):
            return [(np.zeros((0, 18, 3)), np.zeros(0), None)] * n

    fd, hd = _FakeCpm(False), _FakeCpm(True)
    assert wb.detect_staged(_FakePose(Ctx()), fd, hd, 0, 2) == [[], []]
    assert fd.calls == [] and hd.calls == []
