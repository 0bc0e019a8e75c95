"""Training labels from keypoints, host side (no GPU): the float64 NumPy path ``make_labels_np``
against the reference's own generate_heatmaps / generate_pafs / parse_coco_annotation outputs
(tests/golden/labels/, made by tests/golden/make_golden_labels.py), the dilate + ``> 0`` rule of
the ignore mask, and the argument validation of op_make_labels (which runs before any device call).
"""
import ctypes
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN, pkg_module

FRAMES = ("a_0", "a_1", "a_2", "b_0")


def load_frame(name):
    return dict(np.load(os.path.join(GOLDEN, "labels", name + ".npz")))


@pytest.fixture(scope="module")
def labels():
    return pkg_module("labels")


def test_fixture_set_is_complete():
    names = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "labels", "*.npz")))
    assert names == sorted(FRAMES + ("parse",))
    assert [len(load_frame(f)["poses"]) for f in FRAMES] == [0, 3, 17, 5]
    for f in FRAMES:
        assert os.path.getsize(os.path.join(GOLDEN, "labels", f + ".npz")) < 512 * 1024


@pytest.mark.parametrize("name", FRAMES)
def test_full_resolution_matches_the_reference_bit_for_bit(labels, name):
    d = load_frame(name)
    _, h, w = d["heatmaps"].shape
    pafs, heat, ign = labels.make_labels_np([d["poses"]], h, w, downscale=1)
    assert pafs.dtype == np.float32 and heat.dtype == np.float32
    assert np.array_equal(pafs[0], d["pafs"])
    assert np.array_equal(heat[0], d["heatmaps"])
    assert ign.shape == (1, h, w) and not ign.any()


@pytest.mark.parametrize("name", FRAMES)
def test_downscale_8_is_resize_images_of_the_reference_labels(labels, name):
    from oracle import postproc
    d = load_frame(name)
    _, h, w = d["heatmaps"].shape
    pafs, heat, ign = labels.make_labels_np([d["poses"]], h, w, downscale=8)
    assert np.array_equal(pafs[0], postproc.resize_images(d["pafs"], h // 8, w // 8))
    assert np.array_equal(heat[0], postproc.resize_images(d["heatmaps"], h // 8, w // 8))
    assert ign.shape == (1, h // 8, w // 8) and not ign.any()


def test_fixture_a1_has_the_special_limbs():
    """The horizontal, vertical and coincident limbs of case A are what the generator says."""
    p = load_frame("a_1")["poses"]
    assert p[0, 1, 1] == p[0, 8, 1] and p[0, 1, 0] != p[0, 8, 0] and p[0, 1, 2] > 0 and p[0, 8, 2] > 0
    assert p[1, 1, 0] == p[1, 11, 0] and p[1, 1, 1] != p[1, 11, 1] and p[1, 1, 2] > 0 and p[1, 11, 2] > 0
    assert np.array_equal(p[2, 2], p[2, 3]) and p[2, 2, 2] > 0


def test_parse_coco_annotation_matches_the_reference(labels):
    d = dict(np.load(os.path.join(GOLDEN, "labels", "parse.npz")))
    anns = [{"keypoints": [int(v) for v in kp], "num_keypoints": int(nk), "area": float(ar)}
            for kp, nk, ar in zip(d["keypoints"], d["num_keypoints"], d["area"])]
    poses = labels.parse_coco_annotation(anns)
    assert poses.dtype == np.int32 and np.array_equal(poses, d["poses"])
    assert poses[0, 1, 2] == 2 and poses[1, 1, 2] == 0  # Neck: both shoulders / one shoulder
    assert labels.parse_coco_annotation([]).shape == (0, 18, 3)


def test_valid_annotations_filter(labels):
    anns = [{"num_keypoints": 5, "area": 1025.0}, {"num_keypoints": 4, "area": 5000.0},
            {"num_keypoints": 9, "area": 1024.0}]
    assert labels.valid_annotations(anns) == anns[:1]
    assert labels.valid_annotations(anns[1:]) is None


def test_train_params_are_the_reference_entries(labels, pkg):
    tp = labels.train_params
    assert (tp["min_keypoints"], tp["min_area"], tp["insize"], tp["downscale"], tp["paf_sigma"],
            tp["heatmap_sigma"]) == (5, 1024, 368, 8, 8, 7)
    assert (tp["min_box_size"], tp["max_box_size"], tp["min_scale"], tp["max_scale"], tp["max_rotate_degree"],
            tp["center_perterb_max"]) == (64, 512, 0.5, 2.0, 40, 40)
    J = pkg.JointType
    assert [int(j) for j in tp["coco_joint_indices"]] == [int(j) for j in (
        J.Nose, J.LeftEye, J.RightEye, J.LeftEar, J.RightEar, J.LeftShoulder, J.RightShoulder, J.LeftElbow,
        J.RightElbow, J.LeftHand, J.RightHand, J.LeftWaist, J.RightWaist, J.LeftKnee, J.RightKnee, J.LeftFoot,
        J.RightFoot)]


@pytest.mark.parametrize("where", ["first", "last", "interior"])
def test_ignore_mask_dilation_rule(labels, where):
    """A set source pixel s sets destinations s-7 .. s+8 on each axis (cv2.MORPH_DILATE with
    ones((16, 16)), anchor 8), clipped to the image; at the network resolution a pixel is ignored
    when resize_images of the dilated mask is > 0 there."""
    from oracle import postproc
    h, w = 40, 48
    sy, sx = {"first": (0, 0), "last": (h - 1, w - 1), "interior": (17, 22)}[where]
    mask = np.zeros((1, h, w), np.uint8)
    mask[0, sy, sx] = 255
    want = np.zeros((h, w), bool)
    want[max(0, sy - 7):min(h, sy + 9), max(0, sx - 7):min(w, sx + 9)] = True
    empty = [np.zeros((0, 18, 3))]
    _, _, full = labels.make_labels_np(empty, h, w, mask=mask, downscale=1)
    assert full.dtype == bool and np.array_equal(full[0], want)
    _, _, low = labels.make_labels_np(empty, h, w, mask=mask, downscale=8)
    want_low = postproc.resize_images(want[None].astype(np.float32), h // 8, w // 8)[0] > 0
    assert want_low.any() and not want_low.all()
    assert np.array_equal(low[0], want_low)


def _call(lib, n=1, h=40, w=48, downscale=8, poses="default", offsets="default", sigma=7.0, width=8.0):
    if isinstance(poses, str):
        poses = np.ones((2, 18, 3), np.float64)
    if isinstance(offsets, str):
        offsets = np.array([0, 2], np.int32)
    return lib.lib().op_make_labels(0, n, h, w, downscale, lib.ptr(poses), lib.ptr(offsets), None, float(sigma),
                                    float(width), None, None, None)


@pytest.mark.parametrize("kw, word", [
    (dict(poses=None), "null poses"),
    (dict(offsets=None), "pose_offsets"),
    (dict(n=2, offsets=np.array([0, 2, 1], np.int32)), "decrease"),
    (dict(offsets=np.array([1, 2], np.int32)), "pose_offsets[0]"),
    (dict(poses=np.full((2, 18, 3), np.nan)), "non-finite"),
    (dict(poses=np.full((2, 18, 3), np.inf)), "non-finite"),
    (dict(downscale=0), "downscale"),
    (dict(downscale=7), "downscale"),
    (dict(downscale=24), "downscale"),   # 40 / 24 is no integer
    (dict(h=8, w=48, downscale=8), "downscale"),  # h / downscale = 1 < 2
    (dict(sigma=0.0), "heatmap_sigma"),
    (dict(sigma=-1.0), "heatmap_sigma"),
    (dict(sigma=float("nan")), "heatmap_sigma"),
    (dict(width=-1.0), "paf_width"),
    (dict(n=0, offsets=np.array([0], np.int32)), "shape"),
    (dict(h=0), "shape"),
])
def test_op_make_labels_rejects_bad_arguments_without_a_device(lib, kw, word):
    assert _call(lib, **kw) == lib.OP_ERR_INVALID
    assert "op_make_labels" in lib.last_error() and word in lib.last_error(), lib.last_error()


def test_python_wrappers_validate(labels, lib):
    with pytest.raises(ValueError):
        labels.make_labels_np([np.zeros((0, 18, 3))], 40, 48, downscale=7)
    with pytest.raises(ValueError):
        labels.make_labels_np([np.zeros((0, 18, 3))], 40, 48, mask=np.zeros((1, 40, 40)), downscale=8)
    with pytest.raises(ValueError):
        lib.pack_poses([np.zeros((1, 18, 3))], n=2)
    poses, off = lib.pack_poses([np.zeros((2, 18, 3)), np.zeros((0, 18, 3)), np.ones((1, 18, 3), np.int32)])
    assert poses.dtype == np.float64 and poses.shape == (3, 18, 3) and off.tolist() == [0, 2, 2, 3]


def test_export_list_still_equals_the_header(lib):
    import re
    from conftest import REPO
    src = open(os.path.join(REPO, "include", "openpose_hip.h")).read()
    decl = sorted(set(re.findall(r"\b(op_[a-z_]+)\s*\(", src)))
    assert sorted(lib.EXPORTED) == decl
    assert {"op_make_labels", "op_train_step_poses"} <= set(decl)
    L = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(L, "op_make_labels") and hasattr(L, "op_train_step_poses")


def test_synthetic_poses_are_reference_shaped():
    train = pkg_module("train")
    poses = train.synthetic_poses(np.random.default_rng(0), 3, 48, 64, people=4)
    assert len(poses) == 3
    for p in poses:
        assert p.shape == (4, 18, 3) and p.dtype == np.int32
        assert set(np.unique(p[:, :, 2])) <= {0, 1, 2}
