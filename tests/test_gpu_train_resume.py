"""Snapshot / resume on the GPU (op_train_get_state / op_train_set_state, Updater.save_snapshot /
load_snapshot): a run continued from a snapshot takes the very step the uninterrupted run takes,
bit for bit, including Adam's moments and the per-layer step counts that differ once the frozen VGG
layers join in.  The step is deterministic (fixed-order reductions, no atomics); the control run
below checks that first, since everything else here rests on it."""
import numpy as np
import pytest

from conftest import pkg_module

pytestmark = pytest.mark.gpu

N, H, W = 2, 64, 48


@pytest.fixture(scope="module")
def W0():
    return pkg_module("weights").random_weights(seed=7)


def _data(seed):
    from test_gpu_train import _data
    return _data(N, H, W, seed)


def _ctx(weights):
    """The reference's setup: alpha 1e-4, the GradientScaling hook, the VGG layers frozen."""
    T = pkg_module("train")
    ctx = pkg_module("_lib").TrainContext(N, H, W, 0)
    ctx.set_weights(weights)
    ctx.set_hyper(1e-4)
    names = [t[0] for t in ctx.table]
    for nm in T.GRAD_SCALED:
        ctx.set_grad_scale(names.index(nm), 1 / 4)
    for nm in T.VGG_FROZEN:
        ctx.enable(names.index(nm), False)
    return ctx, names


def _enable_vgg(ctx, names):
    for nm in pkg_module("train").VGG_FROZEN:
        ctx.enable(names.index(nm), True)


def _diff(a, b):
    return [k for k in a if not (np.array_equal(a[k][0], b[k][0]) and np.array_equal(a[k][1], b[k][1]))]


def _four_steps(W0, batches, snapshot=False):
    ctx, names = _ctx(W0)
    try:
        ctx.step(*batches[0])
        ctx.step(*batches[1])
        _enable_vgg(ctx, names)
        ctx.step(*batches[2])
        snap = (ctx.get(), ctx.get_state()) if snapshot else None
        losses = ctx.step(*batches[3])
        return ctx.get(), losses, snap
    finally:
        ctx.close()


def test_resume_is_bit_exact(W0):
    T = pkg_module("train")
    batches = [_data(s) for s in (21, 22, 23, 24)]
    W_A, L_A, (W_snap, S_snap) = _four_steps(W0, batches, snapshot=True)
    W_ctl, L_ctl, _ = _four_steps(W0, batches)
    assert not _diff(W_A, W_ctl) and np.array_equal(L_A, L_ctl), \
        "the training step is not deterministic: two identical runs differ in %s" % _diff(W_A, W_ctl)[:5]
    # the snapshot's step counts: the VGG layers joined at the third step
    for name, s in S_snap.items():
        assert s["t"] == (1 if name in T.VGG_FROZEN else 3), (name, s["t"])
        assert s["vW"].any() and s["mW"].any() and s["vW"].min() >= 0, name

    def resumed(with_state):
        ctx, names = _ctx(W_snap)
        try:
            if with_state:
                ctx.set_state(S_snap)
                back = ctx.get_state()
                assert all(back[k]["t"] == S_snap[k]["t"] and np.array_equal(back[k]["mW"], S_snap[k]["mW"])
                           and np.array_equal(back[k]["vb"], S_snap[k]["vb"]) for k in names)
            _enable_vgg(ctx, names)
            losses = ctx.step(*batches[3])
            return ctx.get(), losses
        finally:
            ctx.close()

    W_B, L_B = resumed(True)
    assert np.array_equal(L_B, L_A) and not _diff(W_B, W_A), _diff(W_B, W_A)[:5]
    # without the optimizer state the same step lands elsewhere (fresh moments, t = 1 everywhere):
    # the comparison above can see a lost state
    W_C, L_C = resumed(False)
    assert np.array_equal(L_C, L_A)  # (the loss is the weights' alone)
    assert len(_diff(W_C, W_A)) == len(W_A)


def test_updater_snapshot_round_trip(W0, tmp_path):
    T, weights = pkg_module("train"), pkg_module("weights")
    batches = [(np.random.default_rng(s).integers(0, 256, (N, H, W, 3), dtype=np.uint8),) + _data(s)[1:]
               for s in (31, 32, 33, 34)]
    path = str(tmp_path / "snapshot_iter_3.npz")
    up = T.Updater(N, H, W, model=W0)
    try:
        for b in batches[:3]:
            up.update(b)
        up.save_snapshot(path)
        saved = up.weights()
        want_loss = up.update(batches[3])
        want = up.weights()
    finally:
        up.ctx.close()
    loaded = weights.load_npz(path)  # --initmodel SNAPSHOT
    assert not _diff(loaded, saved)
    up2 = T.Updater(N, H, W, model=weights.random_weights(seed=8), resume=True)  # all of it comes from the file
    try:
        up2.load_snapshot(path)
        assert up2.iteration == 3 and up2.alpha == 1e-4
        assert [n for n in up2.names if not up2.enabled[n]] == T.VGG_FROZEN
        got_loss = up2.update(batches[3])
        got = up2.weights()
        assert up2.iteration == 4
        assert not up2.grads()["conv1_1"][0].any() and up2.grads()["conv4_3_CPM"][0].any()  # frozen again
    finally:
        up2.ctx.close()
    assert got_loss == want_loss and not _diff(got, want), _diff(got, want)[:5]
