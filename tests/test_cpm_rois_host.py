"""ROI detection (FaceDetector / HandDetector.detect_rois), CPU side: the NumPy statement of the
virtual crop against PoseDetector.crop_image, the box helpers against crop_face / crop_hands on the
golden poses, and demo.run(device_crops=True) against the default path with stub detectors."""
import numpy as np

from conftest import load_golden, people_image, pkg_module


def _bare_pose_detector():
    return object.__new__(pkg_module("pose_detector").PoseDetector)  # host-side helpers only


# on a 40 x 50 frame: inside, across each of the four edges, larger on all sides, wholly outside
BOXES = [(5, 7, 31, 30), (-6, 4, 12, 20), (10, -9, 33, 11), (38, 3, 61, 25), (8, 29, 27, 47), (-5, -3, 58, 49),
         (70, 60, 90, 75)]


def test_roi_crop_np_is_crop_image():
    roi_crop_np = pkg_module("face_detector").roi_crop_np
    pd = _bare_pose_detector()
    frame = np.random.default_rng(3).integers(0, 256, (40, 50, 3), dtype=np.uint8)
    for box in BOXES:
        ref = pd.crop_image(frame, box)
        got = roi_crop_np(frame, box, False)
        assert got.dtype == np.uint8 and got.shape == ref.shape == (box[3] - box[1], box[2] - box[0], 3)
        assert np.array_equal(got, ref), box
        assert np.array_equal(roi_crop_np(frame, box, True), ref[:, ::-1]), box
    assert roi_crop_np(frame, BOXES[0]).any() and not roi_crop_np(frame, BOXES[-1]).any()
    # wholly above / left of the frame crop_image raises, like the reference; the statement is zeros
    assert not roi_crop_np(frame, (-30, -40, -3, -2)).any()
    # a row-strided view of a larger array is a frame like any other
    view = np.random.default_rng(4).integers(0, 256, (60, 80, 3), dtype=np.uint8)[5:45, 10:60]
    assert np.array_equal(roi_crop_np(view, BOXES[1], True), pd.crop_image(view, BOXES[1])[:, ::-1])


def test_box_helpers_are_the_crop_functions_boxes():
    pd = _bare_pose_detector()
    img = people_image()
    poses = load_golden("six_people")["poses"]
    n_face = n_hand = n_shift = 0
    for pose in poses:
        unit = pd.get_unit_length(pose)
        a, b = pose.copy(), pose.copy()
        _, fbox = pd.crop_face(img, a, unit)
        assert pd.face_bbox(b, unit) == fbox
        hands = pd.crop_hands(img, a, unit)
        boxes = pd.hand_bboxes(b, unit)
        assert set(boxes) == {"left", "right"}
        for side in ("left", "right"):
            assert boxes[side] == (None if hands[side] is None else hands[side]["bbox"])
            n_hand += boxes[side] is not None
        # the in-place 0.3 elbow->hand shift of the hand rows, and nothing else
        assert np.array_equal(a, b)
        n_shift += not np.array_equal(b, pose)
        n_face += fbox is not None
    assert n_face > 0 and n_hand > 0 and n_shift > 0
    nose_less = poses[0].copy()
    nose_less[0, 2] = 0
    assert pd.face_bbox(nose_less, 10.0) is None


def _stub_scene():
    """demo.run's inputs with stub detectors that serve both paths: detect_rois records its
    arguments and answers through roi_crop_np + the recorded detect_batch stub."""
    roi_crop_np = pkg_module("face_detector").roi_crop_np
    PD = pkg_module("pose_detector").PoseDetector
    img = people_image()
    poses = load_golden("six_people")["poses"]

    class Pose(PD):
        def __init__(self):
            self.device = 0

        def __call__(self, im):
            return poses.copy(), np.ones(len(poses))

    def keypoints(n, crop):
        # a function of the crop's pixels alone
        r = np.random.default_rng(int(crop.astype(np.int64).sum()) + crop.shape[0] * 7 + crop.shape[1])
        return [None if r.random() < 0.2 else [int(r.integers(0, crop.shape[1])), int(r.integers(0, crop.shape[0])),
                                               np.float32(r.random())] for _ in range(n)]

    calls = {"face_batch": [], "hand_batch": [], "face_rois": [], "hand_rois": []}

    class Face(object):
        def detect_batch(self, crops):
            calls["face_batch"].append([c.copy() for c in crops])
            return [keypoints(70, c) for c in crops]

        def detect_rois(self, frame, bboxes, frame_ids=None):
            assert frame is img and frame_ids is None
            calls["face_rois"].append(list(bboxes))
            return self.detect_batch([roi_crop_np(frame, b, False) for b in bboxes])

    class Hand(object):
        def detect_batch(self, crops, sides):
            calls["hand_batch"].append(([c.copy() for c in crops], list(sides)))
            # what HandDetector.detect_batch does with a left hand: the host flip
            return [keypoints(21, c[:, ::-1] if s == "left" else c) for c, s in zip(crops, sides)]

        def detect_rois(self, frame, bboxes, hand_types, frame_ids=None):
            assert frame is img and frame_ids is None
            calls["hand_rois"].append((list(bboxes), list(hand_types)))
            # the device reads a left box mirrored: roi_crop_np(mirror) is the crop detect_batch flips
            for b in bboxes:
                assert np.array_equal(roi_crop_np(frame, b, True), roi_crop_np(frame, b, False)[:, ::-1])
            return self.detect_batch([roi_crop_np(frame, b, False) for b in bboxes], hand_types)

    return img, poses, Pose(), Face(), Hand(), calls


def test_demo_run_device_crops_with_stub_detectors():
    demo = pkg_module("demo")
    img, poses, pd, fd, hd, calls = _stub_scene()
    want = demo.run(img, pd, fd, hd, log=lambda s: None)
    assert len(calls["face_batch"]) == 1 and len(calls["hand_batch"]) == 1 and not calls["face_rois"]
    got = demo.run(img, pd, fd, hd, log=lambda s: None, device_crops=True)
    # one detect_rois call per detector
    assert len(calls["face_rois"]) == 1 and len(calls["hand_rois"]) == 1
    assert len(calls["face_batch"]) == 2 and len(calls["hand_batch"]) == 2
    # exactly the default path's boxes and hand types, in its order
    exp_faces, exp_hands = [], []
    for pose in poses.copy():
        unit = pd.get_unit_length(pose)
        _, fbox = pd.crop_face(img, pose, unit)
        if fbox is not None:
            exp_faces.append(fbox)
        hands = pd.crop_hands(img, pose, unit)
        exp_hands += [(hands[s]["bbox"], s) for s in ("left", "right") if hands[s] is not None]
    assert calls["face_rois"][0] == exp_faces and len(exp_faces) > 0
    assert calls["hand_rois"][0] == ([b for b, _ in exp_hands], [s for _, s in exp_hands])
    assert {s for _, s in exp_hands} == {"left", "right"}
    # and the crops the ROI path stands for are the default path's crops
    for a, b in zip(calls["face_batch"][0], calls["face_batch"][1]):
        assert np.array_equal(a, b)
    assert calls["hand_batch"][0][1] == calls["hand_batch"][1][1]
    for a, b in zip(calls["hand_batch"][0][0], calls["hand_batch"][1][0]):
        assert np.array_equal(a, b)
    assert np.array_equal(got, want) and (got != img).any()
