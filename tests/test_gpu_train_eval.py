"""Validation pass on the GPU (op_train_eval / op_train_eval_poses): the forward and compute_loss of
the training step without its backward and update.  Held to the step itself (the losses a step
reports are the ones before its update, so eval then step on one context must agree bit for bit), to
the float64 torch restatement of tests/test_gpu_train.py for a batch shorter than the context, and to
the reference's own compute_loss values (tests/golden/train/).

Shapes: n=2, 64x48, the existing step test's.  Heat has 2*19*8*6 = 1824 elements and PAF 3648 (m=1:
912 and 1824): neither a multiple of the 256-element block, and the heat tensors fill half the
blocks of the loss kernel's grid."""
import ctypes

import numpy as np
import pytest

from conftest import pkg_module

pytestmark = pytest.mark.gpu

N, H, W = 2, 64, 48


@pytest.fixture(scope="module")
def W0():
    return pkg_module("weights").random_weights(seed=7)


def _ctx(W0=None, n=N, h=H, w=W):
    ctx = pkg_module("_lib").TrainContext(n, h, w, 0)
    if W0 is not None:
        ctx.set_weights(W0)
        ctx.set_hyper(1e-4)
    return ctx


def _data(seed):
    from test_gpu_train import _data
    return _data(N, H, W, seed)


def _same(a, b):
    return all(np.array_equal(a[k][0], b[k][0]) and np.array_equal(a[k][1], b[k][1]) for k in a)


def test_eval_equals_the_following_steps_losses(W0):
    batch = _data(3)
    ctx = _ctx(W0)
    try:
        got = ctx.eval(*batch)
        want = ctx.step(*batch)
    finally:
        ctx.close()
    assert got.shape == (12,) and np.all(got > 0)
    assert np.array_equal(got, want), (got, want)


def test_eval_leaves_the_training_state_alone(W0):
    a, b, c = _data(3), _data(4), _data(5)
    ctx, ctx2 = _ctx(W0), _ctx(W0)
    try:
        ctx.step(*a)
        before = ctx.get(), ctx.get(grads=True), ctx.get_state()
        ctx.eval(*b)
        after = ctx.get(), ctx.get(grads=True), ctx.get_state()
        assert _same(before[0], after[0]) and _same(before[1], after[1])
        assert any(g[0].any() for g in after[1].values())  # the step's gradients, not zeros
        for name, s in before[2].items():
            assert s["t"] == after[2][name]["t"] == 1
            for key in ("mW", "vW", "mb", "vb"):
                assert np.array_equal(s[key], after[2][name][key]), (name, key)
        with pytest.raises(RuntimeError):  # OP_ERR_STATE: no step_poses has run, and eval is not one
            ctx.last_label_ms()
        l1 = ctx.step(*c)
        ctx2.step(*a)
        l2 = ctx2.step(*c)
        assert np.array_equal(l1, l2) and _same(ctx.get(), ctx2.get())
    finally:
        ctx.close()
        ctx2.close()


def test_eval_of_a_shorter_batch_ignores_the_stale_frames(W0):
    """m = 1 < n after a full-batch step on other data: frame 1 of every activation buffer holds the
    step's values, and the result must be the single frame's own losses (float64 torch, the
    tolerance the step's losses are held to)."""
    from test_gpu_train import torch_step
    a, b = _data(3), _data(4)
    ctx = _ctx(W0)
    try:
        ctx.step(*a)
        W1 = ctx.get()
        one = tuple(t[:1] for t in b)
        got = ctx.eval(*one)
        both = ctx.eval(*b)
    finally:
        ctx.close()
    want, _ = torch_step(W1, *one)
    print("eval m=1: max rel loss error vs float64 = %.3g" % float(np.max(np.abs(got - want) / want)))
    np.testing.assert_allclose(got, want, rtol=2e-5)
    assert not np.array_equal(got, both)  # (the second frame does change the mean)


@pytest.mark.parametrize("case", ["posenet_2x48x48", "posenet_1x64x80"])
def test_eval_losses_vs_reference_compute_loss(case):
    from test_train_golden import load_train_case
    from test_forward_golden import case_weights, load_case
    g, _ = load_train_case(case)
    _, d = load_case(case)
    n, h, w = d["x"].shape[0], d["x"].shape[2], d["x"].shape[3]
    ctx = _ctx(None, n, h, w)
    try:
        ctx.set_weights(case_weights("posenet", 0))
        losses = ctx.eval(d["x"], g["pafs_t"], g["heatmaps_t"], g["ignore_mask"])
    finally:
        ctx.close()
    want = np.stack([g["paf_loss"], g["heat_loss"]], 1).reshape(-1)  # [paf, heat] per stage
    print(case, "max rel loss error vs reference compute_loss: %.3g" % float(np.max(np.abs(losses - want) / want)))
    np.testing.assert_allclose(losses, want, rtol=1e-4)


def test_eval_poses_equals_eval_on_the_device_labels_and_step_poses(W0):
    T, labels = pkg_module("train"), pkg_module("labels")
    rng = np.random.default_rng(11)
    x = rng.uniform(-0.5, 0.5, (N, 3, H, W)).astype(np.float32)
    poses = T.synthetic_poses(rng, N, H, W, people=3)
    mask = np.zeros((N, H, W), bool)
    mask[0, 10, 12] = mask[1, 40:44, 30] = True
    sigma, width = labels.train_params["heatmap_sigma"], labels.train_params["paf_sigma"]
    pafs, heat, ign = labels.make_labels(poses, H, W, mask, downscale=8)
    assert ign.any() and not ign.all() and np.abs(pafs).max() > 0
    ctx = _ctx(W0)
    try:
        got = ctx.eval_poses(x, poses, mask, sigma, width)
        assert np.array_equal(got, ctx.eval(x, pafs, heat, ign))
        # a shorter batch: its own offsets and mask frames
        one = ctx.eval_poses(x[:1], poses[:1], mask[:1], sigma, width)
        assert np.array_equal(one, ctx.eval(x[:1], pafs[:1], heat[:1], ign[:1]))
        no_mask = ctx.eval_poses(x, poses, None, sigma, width)
        assert not np.array_equal(no_mask, got)
        with pytest.raises(RuntimeError):  # OP_ERR_STATE: eval_poses is no step_poses
            ctx.last_label_ms()
        assert np.array_equal(got, ctx.step_poses(x, poses, mask, sigma, width))
        assert ctx.last_label_ms() > 0
    finally:
        ctx.close()


def test_argument_errors(W0):
    L = pkg_module("_lib")
    x, pt, ht, ig = _data(3)
    x3, pt3, ht3, ig3 = (np.concatenate([t, t[:1]]) for t in (x, pt, ht, ig))
    losses = np.zeros(12)

    def raw(ctx, m, x=x3, pt=pt3, ht=ht3, ig=ig3, out=losses):
        return L.lib().op_train_eval(ctx.h_, m, L.ptr(x), L.ptr(pt), L.ptr(ht), L.ptr(ig), L.ptr(out))

    ctx = _ctx()
    try:
        assert raw(ctx, 1) == L.OP_ERR_STATE  # before set_weights
        offs = np.zeros(2, np.int32)
        assert L.lib().op_train_eval_poses(ctx.h_, 1, L.ptr(x3), None, L.ptr(offs), None, 7.0, 8.0,
                                           L.ptr(losses)) == L.OP_ERR_STATE
        ctx.set_weights(W0)
        assert raw(ctx, 0) == L.OP_ERR_INVALID and raw(ctx, 3) == L.OP_ERR_INVALID and raw(ctx, -1) == L.OP_ERR_INVALID
        assert "1 <= m <= n" in L.last_error()
        assert raw(ctx, 2, x=None) == L.OP_ERR_INVALID and raw(ctx, 2, pt=None) == L.OP_ERR_INVALID
        assert raw(ctx, 2, ig=None) == L.OP_ERR_INVALID and raw(ctx, 2, out=None) == L.OP_ERR_INVALID
        assert L.lib().op_train_eval_poses(ctx.h_, 3, L.ptr(x3), None, L.ptr(np.zeros(4, np.int32)), None, 7.0, 8.0,
                                           L.ptr(losses)) == L.OP_ERR_INVALID
        with pytest.raises(ValueError):  # the wrapper refuses m > n itself
            ctx.eval(x3, pt3, ht3, ig3)
        with pytest.raises(ValueError):
            ctx.eval(x, pt[:1], ht, ig)
        assert raw(ctx, 2) == L.OP_OK and np.all(losses > 0)
        # set_state: every pointer, no negative step count
        state = ctx.get_state()
        state["conv1_1"]["t"] = -1
        with pytest.raises(ValueError):
            ctx.set_state(state)
        nl = len(ctx.table)
        null = (ctypes.c_void_p * nl)()
        t = np.zeros(nl, np.int64)
        assert L.lib().op_train_set_state(ctx.h_, null, null, null, null, L.ptr(t)) == L.OP_ERR_INVALID
        assert L.lib().op_train_set_state(ctx.h_, None, None, None, None, L.ptr(t)) == L.OP_ERR_INVALID
        # get_state: null arrays and entries are skipped
        assert L.lib().op_train_get_state(ctx.h_, None, null, None, None, L.ptr(t)) == L.OP_OK
        assert not t.any()
    finally:
        ctx.close()
