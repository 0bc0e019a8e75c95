"""Display lists on the device (op_draw / op_draw_staged, csrc/draw.hip) against the statement
render.render_np: every comparison is exact."""
import ctypes
import os
import time

import numpy as np
import pytest

from conftest import GOLDEN, load_golden, people_image, pkg_module

pytestmark = pytest.mark.gpu

COLORS = [(0, 255, 0), (255, 85, 0), (0, 0, 255), (170, 0, 255), (255, 255, 0), (1, 2, 3), (255, 255, 255)]
# (dx, dy) of thickness-2 lines on which an exact-integer distance test paints extra tie pixels
TIES = [(8, 6), (6, 8), (12, 5), (12, 9)]


@pytest.fixture(scope="module")
def render():
    return pkg_module("render")


def frame(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def check(render, imgs, lists):
    keep = [a.copy() for a in imgs]
    got = render.render(imgs, lists)
    assert len(got) == len(imgs)
    for i, (img, prims) in enumerate(zip(imgs, lists)):
        want = render.render_np(img, prims)
        assert got[i].shape == img.shape and got[i].dtype == np.uint8
        assert np.array_equal(got[i], want), (i, np.argwhere((got[i] != want).any(axis=2))[:8])
        assert np.array_equal(img, keep[i])
    return got


def tie_lines(R, origins):
    prims = []
    for k, (ox, oy) in enumerate(origins):
        for j, (dx, dy) in enumerate(TIES):
            for sx, sy in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
                for t in (2, 1):
                    prims.append(R.LINE(float(ox), float(oy), float(ox + sx * dx), float(oy + sy * dy), float(t),
                                        COLORS[(k + j + t) % len(COLORS)]))
    return prims


def two_people(R, h, w):
    """Two overlapping people in draw_person_pose's order: limbs, then discs over them; the second
    person's limbs cross the first's."""
    poses = np.zeros((2, 18, 3))
    rng = np.random.default_rng(3)
    base = np.stack([rng.uniform(0.1 * w, 0.9 * w, 18), rng.uniform(0.1 * h, 0.9 * h, 18)], axis=1)
    poses[0, :, :2] = base
    poses[1, :, :2] = base[::-1] * 0.5 + base * 0.5 + 2.0
    poses[:, :, 2] = 2
    poses[1, 4, 2] = 0
    return R.pose_list(poses)


def test_mixed_batch_in_one_call(render):
    R = render
    imgs = [frame(1, 33, 17), frame(2, 75, 101), frame(3, 96, 128)]
    small = tie_lines(R, [(8, 16), (3, 30)])
    small += [R.LINE(5.0, 5.0, 5.0, 5.0, 2.0, COLORS[0]), R.LINE(9.0, 9.0, 9.0, 9.0, 1.0, COLORS[1]),  # zero length
              R.DISC(16, 32, 0, COLORS[2]), R.DISC(0, 0, 0, COLORS[3]), R.DISC(17, 5, 0, COLORS[4]),   # radius 0; one off
              R.DISC(-2, 10, 3, COLORS[5]), R.LINE(-5.0, 20.0, 30.0, 28.0, 2.0, COLORS[6])]
    mid = tie_lines(R, [(50, 40), (64, 16), (20, 60)])
    rng = np.random.default_rng(7)
    for k in range(40):  # float end points, 1 px, as the hand and face drawers pass them
        a, b = rng.uniform(-8, 110, 2), rng.uniform(-8, 84, 2)
        mid.append(R.LINE(float(a[0]), float(b[0]), float(a[1]), float(b[1]), 1.0, COLORS[k % len(COLORS)]))
    mid += [R.LINE(10.25, 10.5, 10.25, 10.5, 1.0, COLORS[2]), R.LINE(30.5, 20.5, 34.5, 20.5, 1.0, COLORS[3]),
            R.LINE(-40.0, -40.0, -20.0, -30.0, 2.0, COLORS[0]), R.LINE(300.0, 10.0, 400.0, 90.0, 2.0, COLORS[1]),  # wholly off
            R.DISC(200, 200, 3, COLORS[2]), R.DISC(-30, 40, 3, COLORS[3]), R.DISC(100, 74, 3, COLORS[4]),
            R.DISC(50, -2, 3, COLORS[5]), R.DISC(63, 15, 6, COLORS[6]), R.DISC(64, 16, 0, COLORS[0]),
            R.LINE(-20.0, 30.0, 130.0, 47.0, 2.0, COLORS[1]), R.LINE(70.0, -10.0, 60.0, 90.0, 3.0, COLORS[2])]
    big = two_people(R, 96, 128) + [R.BLEND(0.6, 0.4, 0)] + tie_lines(R, [(64, 48), (127, 95)])
    got = check(render, imgs, [small, mid, big])
    assert all((g != i).any() for g, i in zip(got, imgs))
    # order matters: the same primitives reversed draw another picture, and the device follows
    rev = check(render, [imgs[2]], [two_people(R, 96, 128)[::-1]])[0]
    assert (rev != check(render, [imgs[2]], [two_people(R, 96, 128)])[0]).any()


def long_list(R, n, h, w, seed):
    rng = np.random.default_rng(seed)
    prims = []
    for k in range(n):
        c = tuple(int(v) for v in rng.integers(0, 256, 3))
        if k % 3 == 2:
            prims.append(R.DISC(int(rng.integers(-4, w + 4)), int(rng.integers(-4, h + 4)), int(rng.integers(0, 6)), c))
        elif k % 3 == 1:  # short lines about the tile corners (multiples of 64 x 16)
            cx, cy = 64 * int(rng.integers(0, w // 64 + 1)), 16 * int(rng.integers(0, h // 16 + 1))
            a, b = rng.integers(-9, 10, 2), rng.integers(-9, 10, 2)
            prims.append(R.LINE(float(cx + a[0]), float(cy + b[0]), float(cx + a[1]), float(cy + b[1]),
                                float(rng.integers(1, 4)), c))
        else:
            a, b = rng.uniform(-5, w + 5, 2), rng.uniform(-5, h + 5, 2)
            prims.append(R.LINE(float(a[0]), float(b[0]), float(a[1]), float(b[1]), 1.0, c))
    return prims


@pytest.mark.parametrize("blend_at", [None, 300, 0, 900])
def test_lists_longer_than_a_chunk(render, blend_at):
    """900 primitives: four chunks of the kernel's 256, the last 300 all crossing tile (0, 0) (a chunk
    whose every primitive survives the cull); the blend marker inside a chunk, first and last."""
    R = render
    prims = long_list(R, 600, 96, 128, 17)
    prims += [R.LINE(0.0, 0.0, 127.0, 95.0, 2.0, COLORS[k % 7]) for k in range(300)]  # every one hits tile (0, 0)
    if blend_at is not None:
        prims.insert(blend_at, R.BLEND(0.3, 0.7, 2.0))
    check(render, [frame(4, 96, 128), frame(5, 50, 70)], [prims, prims[::-1]])


def test_empty_list_and_blend_only(render):
    R, demo = render, pkg_module("demo")
    imgs = [frame(6, 33, 17), frame(8, 75, 101), frame(9, 20, 130)]
    got = check(render, imgs, [[], [R.BLEND(0.6, 0.4, 0)], [R.BLEND(1.5, 0.75, -20.25)]])
    assert np.array_equal(got[0], imgs[0])
    assert np.array_equal(got[1], demo.add_weighted(imgs[1], 0.6, imgs[1], 0.4, 0))
    assert np.array_equal(got[2], demo.add_weighted(imgs[2], 1.5, imgs[2], 0.75, -20.25))
    assert got[2].max() == 255 and got[2].min() == 0  # both ends saturate
    # ties of rint: 0.5 * a + 0.5 * b + 0 is a half for every odd a + b
    a = frame(10, 40, 64)
    b = [R.LINE(0.0, float(y), 63.0, float(y), 1.0, (y, 255 - y, 7)) for y in range(40)]
    check(render, [a], [b + [R.BLEND(0.5, 0.5, 0.0)]])


def synthetic_people(n, h, w, seed):
    rng = np.random.default_rng(seed)
    poses = np.zeros((n, 18, 3))
    poses[:, :, 0] = rng.uniform(0, w, (n, 18))
    poses[:, :, 1] = rng.uniform(0, h, (n, 18))
    poses[:, :, 2] = 2
    return poses


def test_staged_frames_are_drawn_in_place(render, lib, rand_weights):
    R = render
    limits = lib.OpLimits()
    limits.max_batch = 3
    c = lib.Context(0, None, limits)
    try:
        c.set_weights(rand_weights)
        assert c.staged_info() == (0, 0, 0)
        frames = np.stack([frame(20 + i, 96, 128) for i in range(3)])
        c.stage_frames(frames)
        assert c.staged_info() == (3, 96, 128)
        c.run_staged()
        c.synchronize()
        first = c.fetch_results(0, 3)
        lists = [R.pose_list(p) + [R.BLEND(0.6, 0.4, 0)] for p, _, _ in first]
        out = R.render_staged(c, 0, 3, lists)
        assert out.shape == (3, 96, 128, 3) and out.dtype == np.uint8
        for i in range(3):
            assert np.array_equal(out[i], R.render_np(frames[i], lists[i]))
        # random weights find few people: people of our own on frames 1 and 2, queued behind a run
        own = [R.pose_list(synthetic_people(3, 96, 128, 30 + i)) + [R.BLEND(0.6, 0.4, 0)] for i in range(2)]
        c.run_staged()
        out = R.render_staged(c, 1, 2, own)
        for i in range(2):
            assert np.array_equal(out[i], R.render_np(frames[1 + i], own[i]))
        assert R.last_ms() > 0
        c.synchronize()
        again = c.fetch_results(0, 3)
        for (p0, s0, r0), (p1, s1, r1) in zip(first, again):  # the staged frames were not modified
            assert np.array_equal(p0, p1) and np.array_equal(s0, s1) and r0.n_peaks == r1.n_peaks
        for bad_first, bad_n in ((-1, 1), (3, 1), (2, 2), (0, 4)):
            with pytest.raises(ValueError, match="staged"):
                R.render_staged(c, bad_first, bad_n, [[]] * bad_n)
        with pytest.raises(ValueError, match="thickness"):
            R.render_staged(c, 0, 1, [[R.LINE(0.0, 0.0, 1.0, 1.0, 0.0, COLORS[0])]])
    finally:
        c.close()


def test_staged_draw_with_nothing_staged(render, lib):
    c = lib.Context(0)
    try:
        off, cprims = render.pack_lists([[]])
        out = np.zeros(16, np.uint8)
        assert lib.lib().op_draw_staged(c.h, 0, 1, lib.ptr(off), cprims, lib.ptr(out)) == lib.OP_ERR_STATE
        assert "staged" in lib.last_error()
        with pytest.raises(RuntimeError, match="staged"):
            render.render_staged(c, 0, 1, [[]])
    finally:
        c.close()


def test_demo_device_draw_is_the_host_drawing():
    demo, W = pkg_module("demo"), pkg_module("weights")
    pd = pkg_module("pose_detector").PoseDetector("posenet", model=W.random_weights(0))
    hd = pkg_module("hand_detector").HandDetector("handnet", model=W.random_weights(0, arch="handnet"))
    fd = pkg_module("face_detector").FaceDetector("facenet", model=W.random_weights(0, arch="facenet"))
    img = pkg_module("draw").read_bgr(os.path.join(GOLDEN, "person.png"))
    quiet = lambda s: None
    host = demo.run(img, pd, fd, hd, log=quiet)
    dev = demo.run(img, pd, fd, hd, log=quiet, device_draw=True)
    assert dev.shape == img.shape and dev.dtype == np.uint8 and np.array_equal(dev, host)
    # random weights find nobody: the six golden people on people.png exercise faces, hands and boxes
    poses = load_golden("six_people")["poses"]

    class Pose(object):
        def __call__(self, im):
            return poses.copy(), np.ones(len(poses))

        def __getattr__(self, name):
            return getattr(pd, name)

    img = people_image()
    host = demo.run(img, Pose(), fd, hd, log=quiet)
    dev = demo.run(img, Pose(), fd, hd, log=quiet, device_draw=True)
    assert np.array_equal(dev, host) and (dev != img).any()


def test_timing_of_eight_frames(render):
    """Prints the device time (op_draw_last_ms: uploads + kernel) and the host time of render_np on
    the same input: 8 frames of 368 x 368 with 4 people each.  No threshold: the device time is
    positive."""
    R = render
    imgs = [frame(40 + i, 368, 368) for i in range(8)]
    lists = [R.pose_list(synthetic_people(4, 368, 368, 50 + i)) + [R.BLEND(0.6, 0.4, 0)] for i in range(8)]
    R.render(imgs, lists)  # first call: module load
    times = []
    for _ in range(5):
        got = R.render(imgs, lists)
        times.append(R.last_ms())
    t0 = time.perf_counter()
    want = [R.render_np(a, l) for a, l in zip(imgs, lists)]
    host_ms = (time.perf_counter() - t0) * 1e3
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    print("\nop_draw_last_ms (8 x 368 x 368, 4 people each): median %.3f ms, min %.3f, max %.3f of 5; render_np %.1f ms"
          % (float(np.median(times)), min(times), max(times), host_ms))
    ms = ctypes.c_double()
    assert lib_ok(ms) and min(times) > 0


def lib_ok(ms):
    L = pkg_module("_lib")
    return L.lib().op_draw_last_ms(0, ctypes.byref(ms)) == L.OP_OK and ms.value > 0
