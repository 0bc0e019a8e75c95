"""Training labels on the GPU (op_make_labels, csrc/labels.hip) against the reference's own
generate_pafs / generate_heatmaps outputs (tests/golden/labels/) and, at the network resolution,
oracle.resize_images of them; the ignore mask against the NumPy restatement (itself pinned to the
dilation rule in test_labels_host.py); and op_train_step_poses against op_train_step.

Bounds.  PAFs use only float64 add / multiply / divide / compare in the reference's order: bit-exact
at both resolutions.  Heat maps go through exp: the device's float64 exp and NumPy's may differ in
the last float64 ulp, so the f32 cast can land on the neighbouring f32 value; values are in [0, 1],
where neighbours differ by at most 2^-24, hence |err| <= 2^-23 at full resolution.  At downscale 8
each output is a four-tap f32 sum (weights sum to 1) of such values plus under seven half-ulp
roundings: |err| <= 2^-22.  The tests print how many elements are not identical.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN, pkg_module

pytestmark = pytest.mark.gpu

A, B = ("a_0", "a_1", "a_2"), ("b_0",)


def load_frame(name):
    return dict(np.load(os.path.join(GOLDEN, "labels", name + ".npz")))


def _mask(seed, n, h, w):
    """A few single pixels (corners among them) and one block per frame; frame 0 stays empty."""
    rng = np.random.default_rng(seed)
    m = np.zeros((n, h, w), np.uint8)
    for f in range(1, n):
        ys, xs = rng.integers(0, h, 3), rng.integers(0, w, 3)
        m[f, ys, xs] = 255
        m[f, h - 1, 0] = 1
        m[f, 10:14, 20:29] = 7
    if n == 1:
        m[0, 0, w - 1] = 255
        m[0, 40, 30] = 1
    return m


@pytest.fixture(scope="module")
def cases():
    """{case: (frames, h, w, mask)} from the fixtures."""
    out = {}
    for name, frames in (("A", A), ("B", B)):
        fr = [load_frame(f) for f in frames]
        _, h, w = fr[0]["heatmaps"].shape
        out[name] = (fr, h, w, _mask(len(name) + h, len(fr), h, w))
    return out


@pytest.fixture(scope="module")
def gpu(cases):
    """{(case, downscale): (pafs, heatmaps, ignore)}: one device call per entry, shared by the tests."""
    labels = pkg_module("labels")
    return {(name, ds): labels.make_labels([f["poses"] for f in fr], h, w, mask=mask, downscale=ds)
            for name, (fr, h, w, mask) in cases.items() for ds in (1, 8)}


@pytest.fixture(scope="module")
def want(cases):
    """{(case, downscale): (pafs, heatmaps)} of the reference (downscale 8: oracle.resize_images of it)."""
    from oracle import postproc
    out = {}
    for name, (fr, h, w, _) in cases.items():
        out[name, 1] = (np.stack([f["pafs"] for f in fr]), np.stack([f["heatmaps"] for f in fr]))
        out[name, 8] = tuple(np.stack([postproc.resize_images(f[k], h // 8, w // 8) for f in fr])
                             for k in ("pafs", "heatmaps"))
    return out


@pytest.mark.parametrize("ds", [1, 8])
@pytest.mark.parametrize("case", ["A", "B"])
def test_pafs_bit_exact(gpu, want, case, ds):
    got, ref = gpu[case, ds][0], want[case, ds][0]
    assert got.shape == ref.shape and got.dtype == np.float32
    assert np.abs(ref).max() > 0.5  # the case has limbs
    print("pafs %s downscale %d: %d of %d elements differ" % (case, ds, int((got != ref).sum()), ref.size))
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("ds, bound", [(1, 2.0 ** -23), (8, 2.0 ** -22)])
@pytest.mark.parametrize("case", ["A", "B"])
def test_heatmaps_within_the_exp_bound(gpu, want, case, ds, bound):
    got, ref = gpu[case, ds][1], want[case, ds][1]
    assert got.shape == ref.shape and got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    print("heatmaps %s downscale %d: %d of %d elements not identical, max |err| %.3g (bound %.3g)" % (
        case, ds, int((got != ref).sum()), ref.size, err.max(), bound))
    assert err.max() <= bound


@pytest.mark.parametrize("ds", [1, 8])
@pytest.mark.parametrize("case", ["A", "B"])
def test_ignore_mask_exact(gpu, cases, case, ds):
    labels = pkg_module("labels")
    fr, h, w, mask = cases[case]
    empty = [np.zeros((0, 18, 3))] * len(fr)
    ref = labels.make_labels_np(empty, h, w, mask=mask, downscale=ds)[2]
    got = gpu[case, ds][2]
    assert got.dtype == bool and got.shape == ref.shape
    assert ref.any() and not ref.all()
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("ds", [1, 8])
def test_null_mask_ignores_nothing(cases, gpu, ds):
    labels = pkg_module("labels")
    fr, h, w, _ = cases["B"]
    pafs, heat, ign = labels.make_labels([f["poses"] for f in fr], h, w, mask=None, downscale=ds)
    assert ign.shape == (1, h // ds, w // ds) and not ign.any()
    assert np.array_equal(pafs, gpu["B", ds][0]) and np.array_equal(heat, gpu["B", ds][1])


@pytest.mark.parametrize("ds", [1, 8])
def test_batch_equals_frames_run_singly(cases, gpu, ds):
    labels = pkg_module("labels")
    fr, h, w, mask = cases["A"]
    for i, f in enumerate(fr):
        single = labels.make_labels([f["poses"]], h, w, mask=mask[i:i + 1], downscale=ds)
        for got, batch in zip(single, gpu["A", ds]):
            assert np.array_equal(got[0], batch[i])


def test_step_poses_equals_step_on_device_made_labels(lib, rand_weights):
    """Both paths run the same kernels on the same device buffers: every loss, gradient and
    updated weight is bit-identical."""
    labels, train = pkg_module("labels"), pkg_module("train")
    n, h, w = 2, 48, 48
    rng = np.random.default_rng(3)
    x = rng.uniform(-0.5, 0.5, (n, 3, h, w)).astype(np.float32)
    poses = train.synthetic_poses(rng, n, h, w, people=3)
    mask = rng.random((n, h, w)) < 0.002
    pafs, heat, ign = labels.make_labels(poses, h, w, mask=mask, downscale=8)
    assert np.abs(pafs).max() > 0 and ign.any() and not ign.all()
    out = []
    for use_poses in (False, True):
        ctx = lib.TrainContext(n, h, w)
        try:
            ctx.set_weights(rand_weights)
            losses = ctx.step_poses(x, poses, mask) if use_poses else ctx.step(x, pafs, heat, ign)
            label_ms = ctx.last_label_ms() if use_poses else None
            out.append((losses, ctx.get(grads=True), ctx.get()))
        finally:
            ctx.close()
    assert label_ms is not None and label_ms > 0
    (l0, g0, w0), (l1, g1, w1) = out
    assert l0.shape == (12,) and np.all(l0 > 0)
    assert np.array_equal(l0, l1)
    for name in g0:
        for k in (0, 1):
            assert np.array_equal(g0[name][k], g1[name][k]), name
            assert np.array_equal(w0[name][k], w1[name][k]), name
