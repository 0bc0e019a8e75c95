"""Display lists (render.py) on the host: the lists equal the reference's recorded draw calls, the
statement ``render_np`` equals draw.py / demo.py, and the C ABI's struct and validation (which runs
before any device call: no GPU needed)."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, REPO, pkg_module


@pytest.fixture(scope="module")
def render():
    return pkg_module("render")


with open(os.path.join(GOLDEN, "draw_calls.json")) as _f:
    DRAW_CASES = json.load(_f)


@pytest.mark.parametrize("case", sorted(DRAW_CASES))
def test_pose_list_is_the_recorded_call_sequence(render, case):
    """tests/golden/draw_calls.json holds the reference's own cv2.line / cv2.circle calls per case;
    the display list, turned back into calls, is that sequence."""
    c = DRAW_CASES[case]
    prims = render.pose_list(np.asarray(c["poses"], np.float64).reshape(-1, 18, 3))
    want = [{k: v for k, v in call.items() if k != "canvas"} for call in c["calls"]]
    assert render.calls(prims) == want
    assert all(isinstance(p, (render.LINE, render.DISC)) for p in prims)


def random_people(rng, n, h, w):
    """n poses over (and beyond) an h x w canvas: a third of the joints undetected, some off the canvas."""
    poses = np.zeros((n, 18, 3))
    poses[:, :, 0] = rng.uniform(-0.3 * w, 1.3 * w, (n, 18))
    poses[:, :, 1] = rng.uniform(-0.3 * h, 1.3 * h, (n, 18))
    poses[:, :, 2] = rng.integers(0, 3, (n, 18))
    return poses


def test_render_np_equals_the_pose_blend(render):
    D, demo = pkg_module("draw"), pkg_module("demo")
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (75, 101, 3), dtype=np.uint8)
    poses = random_people(rng, 3, 75, 101)
    assert (poses[:, :, 2] == 0).any() and (poses[:, :, 0] < 0).any() and (poses[:, :, 1] > 75).any()
    keep = img.copy()
    got = render.render_np(img, render.pose_list(poses) + [render.BLEND(0.6, 0.4, 0)])
    want = demo.add_weighted(img, 0.6, D.draw_person_pose(img, poses), 0.4, 0)
    assert np.array_equal(img, keep)
    assert np.array_equal(got, want) and (got != img).any()
    # without the marker: the drawing itself
    assert np.array_equal(render.render_np(img, render.pose_list(poses)), D.draw_person_pose(img, poses))
    assert np.array_equal(render.render_np(img, []), img)
    with pytest.raises(ValueError, match="BLEND"):
        render.render_np(img, [render.BLEND(1, 0, 0), render.BLEND(1, 0, 0)])


def demo_scene():
    """A 2-person scene for demo.run with stub detectors: (img, poses, stub pose / face / hand
    detectors, the keypoints they return).  Person 1 has no nose: no face crop."""
    PD = pkg_module("pose_detector").PoseDetector
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (120, 160, 3), dtype=np.uint8)
    poses = np.zeros((2, 18, 3))
    for p, ox in enumerate((30.0, 95.0)):
        poses[p, :, 0] = ox + rng.uniform(-20, 40, 18)
        poses[p, :, 1] = 10 + rng.uniform(0, 100, 18)
        poses[p, :, 2] = 2
    poses[1, 0, 2] = 0   # person 1: nose not detected
    poses[1, 7, 2] = 0   # and no left hand
    poses[0, 16, 2] = 0

    class Pose(PD):
        def __init__(self):
            self.device = 0

        def __call__(self, im):
            return poses.copy(), np.ones(len(poses))

    def keypoints(n, seed, side):
        r = np.random.default_rng(seed)
        return [None if r.random() < 0.2 else [int(r.integers(0, side)), int(r.integers(0, side)), np.float32(r.random())]
                for _ in range(n)]

    served = {"face": [], "hand": []}

    class Face(object):
        def detect_batch(self, crops):
            out = [keypoints(70, 100 + i, max(c.shape[0], 2)) for i, c in enumerate(crops)]
            served["face"] += out
            return out

    class Hand(object):
        def detect_batch(self, crops, sides):
            out = [keypoints(21, 200 + i, max(c.shape[0], 2)) for i, c in enumerate(crops)]
            served["hand"] += list(zip(sides, out))
            return out

    return img, poses, Pose(), Face(), Hand(), served


def test_demo_list_is_demo_run(render):
    demo = pkg_module("demo")
    img, poses, pd, fd, hd, served = demo_scene()
    want = demo.run(img, pd, fd, hd, log=lambda s: None)
    assert len(served["face"]) == 1 and [s for s, _ in served["hand"]] == ["left", "right", "right"]
    # the same crops, and the stubs' keypoints, as demo.run saw them
    faces, hands = [], []
    face_kps, hand_kps = iter(served["face"]), iter(served["hand"])
    crop_poses = poses.copy()
    for pose in crop_poses:
        unit = pd.get_unit_length(pose)
        crop, bbox = pd.crop_face(img, pose, unit)
        faces.append(None if crop is None else (next(face_kps), bbox))
        ph = pd.crop_hands(img, pose, unit)
        hands.append({s: None if ph[s] is None else (next(hand_kps)[1], ph[s]["bbox"]) for s in ("left", "right")})
    assert faces[1] is None and hands[1]["left"] is None
    prims = render.demo_list(poses, faces, hands)
    assert sum(isinstance(p, render.BLEND) for p in prims) == 1
    got = render.render_np(img, prims)
    assert np.array_equal(got, want) and (got != img).any()


HEADER = os.path.join(REPO, "include", "openpose_hip.h")


def test_op_draw_prim_mirrors_the_header(lib, tmp_path):
    """Size and field offsets of _lib.OpDrawPrim against the C compiler's for op_draw_prim."""
    fields = [n for n, _ in lib.OpDrawPrim._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "openpose_hip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(op_draw_prim));\n' +
                   "".join('  printf(" %%zu", offsetof(op_draw_prim, %s));\n' % f for f in fields) +
                   "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(lib.OpDrawPrim) == 80
    assert got[1:] == [getattr(lib.OpDrawPrim, f).offset for f in fields]
    text = open(HEADER).read()
    for name, value in (("OP_DRAW_LINE", lib.OP_DRAW_LINE), ("OP_DRAW_DISC", lib.OP_DRAW_DISC),
                        ("OP_DRAW_BLEND", lib.OP_DRAW_BLEND)):
        assert "#define %s %d\n" % (name, value) in text


def _op_draw(lib, render, lists, n=None, hw=None, drop=(), offsets=None, stride=None):
    """op_draw on 8 x 8 frames with the given lists -> (rc, message); never reaches a device when an
    argument is bad."""
    k = len(lists)
    imgs = [np.zeros((8, 8, 3), np.uint8) for _ in range(k)]
    outs = [np.zeros((8, 8, 3), np.uint8) for _ in range(k)]
    off, cprims = render.pack_lists(lists)
    if offsets is not None:
        off = np.asarray(offsets, np.int32)
    strides = np.array([24 if stride is None else stride] * k, np.int64)  # kept alive over the call
    sizes = np.array([[8, 8]] * k if hw is None else hw, np.int32)
    args = {"bgr": (ctypes.c_void_p * k)(*[a.ctypes.data for a in imgs]),
            "row_stride": lib.ptr(strides), "hw": lib.ptr(sizes),
            "prim_offsets": lib.ptr(off), "prims": cprims,
            "out": (ctypes.c_void_p * k)(*[a.ctypes.data for a in outs])}
    for name in drop:
        args[name] = None
    rc = lib.lib().op_draw(0, k if n is None else n, args["bgr"], args["row_stride"], args["hw"], args["prim_offsets"],
                           args["prims"], args["out"])
    return rc, lib.last_error()


def test_op_draw_rejects_bad_arguments(lib, render):
    """Every check runs before the first device call: this passes on a machine without a device."""
    LINE, DISC, BLEND = render.LINE, render.DISC, render.BLEND
    col = (1, 2, 3)
    ok = [LINE(1.0, 1.0, 5.0, 4.0, 2.0, col), DISC(3, 3, 2, col), BLEND(0.6, 0.4, 0.0)]

    def bad(word, lists, **kw):
        rc, msg = _op_draw(lib, render, lists, **kw)
        assert rc == lib.OP_ERR_INVALID and "op_draw" in msg and word in msg, (word, rc, msg)

    bad("BLEND", [ok + [BLEND(0.5, 0.5, 0.0)]])
    bad("BLEND", [ok, [BLEND(1.0, 0.0, 0.0), ok[0], BLEND(0.5, 0.5, 0.0)]])
    for field in range(4):
        for value in (np.nan, np.inf, -np.inf, 32768.5, -40000.0):
            v = [1.0, 1.0, 5.0, 4.0]
            v[field] = value
            bad("x0, y0, x1, y1", [[LINE(v[0], v[1], v[2], v[3], 2.0, col)]])
    for value in (0.0, -1.0, np.nan, np.inf, 32769.0):
        bad("thickness", [[LINE(1.0, 1.0, 5.0, 4.0, value, col)]])
    bad("primitive 4", [ok, [ok[0], LINE(1.0, 1.0, 5.0, 4.0, 0.0, col)]])  # a later frame's is checked too, and named
    bad("radius", [[DISC(3, 3, -1, col)]])
    bad("radius", [[DISC(3, 3, 1025, col)]])
    bad("x0, y0", [[DISC(40000, 3, 1, col)]])
    for value in (np.nan, np.inf):
        bad("wa, wb, gamma", [[BLEND(value, 0.4, 0.0)]])
        bad("wa, wb, gamma", [[BLEND(0.6, value, 0.0)]])
        bad("wa, wb, gamma", [[BLEND(0.6, 0.4, value)]])
    # a disc centre must be a whole number; the kind must be known
    _, cprims = render.pack_lists([ok])
    cprims[1].x0 = 3.5
    cprims[0].kind = 7
    off = np.array([0, 3], np.int32)
    img = np.zeros((8, 8, 3), np.uint8)
    one = (ctypes.c_void_p * 1)(img.ctypes.data)
    strides, sizes = np.array([24], np.int64), np.array([8, 8], np.int32)
    call = lambda: lib.lib().op_draw(0, 1, one, lib.ptr(strides), lib.ptr(sizes), lib.ptr(off), cprims, one)
    assert call() == lib.OP_ERR_INVALID and "unknown kind 7" in lib.last_error()
    cprims[0].kind = lib.OP_DRAW_LINE
    assert call() == lib.OP_ERR_INVALID and "whole number" in lib.last_error()
    bad("n must", [ok], n=0)
    bad("n must", [ok], n=-2)
    for name in ("bgr", "row_stride", "hw", "prim_offsets", "prims", "out"):
        bad("null " + name, [ok], drop=(name,))
    for hw in ([0, 8], [8, 0], [16385, 8], [8, 16385], [-1, 8]):
        bad("hw", [ok], hw=[hw])
    bad("row_stride", [ok], stride=23)
    bad("prim_offsets", [ok], offsets=[1, 3])
    bad("prim_offsets", [ok, ok], offsets=[0, 4, 3])
    ms = ctypes.c_double()
    assert lib.lib().op_draw_last_ms(0, None) == lib.OP_ERR_INVALID
    assert lib.lib().op_draw_last_ms(-1, ctypes.byref(ms)) == lib.OP_ERR_INVALID
    assert lib.lib().op_draw_last_ms(64, ctypes.byref(ms)) == lib.OP_ERR_INVALID
    assert lib.lib().op_draw_staged(None, 0, 1, lib.ptr(off), cprims, one) == lib.OP_ERR_INVALID


def test_display_list_refuses_what_draw_refuses(render):
    dl = render.DisplayList()
    with pytest.raises(ValueError):
        dl.circle(None, (1, 1), 3, (0, 0, 0), 1)   # an outlined circle: draw.Raster refuses it too
    with pytest.raises(ValueError):
        dl.circle(None, (1.5, 1), 3, (0, 0, 0), -1)
    dl.line(None, (np.int32(1), np.int32(2)), (3.5, 4), [0, 255.4, 85], 2)
    assert dl.prims == [render.LINE(1.0, 2.0, 3.5, 4.0, 2.0, (0, 255, 85))]
