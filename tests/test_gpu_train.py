"""Training iteration on the GPU against an independent float64 torch autograd
restatement of train_coco_pose_estimation.py:42-123 (CocoPoseNet.__call__ with every stage's maps,
compute_loss with the ignore mask, backward) and of Chainer's Adam + GradientScaling hook.  torch
is the checker here only (tests); the product path is op_train_step."""
import numpy as np
import pytest

from conftest import pkg_module
from train_layerwise import data as _data, hook_multipliers as _hook_multipliers, torch_step  # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def adam_ref(p, g, scale, t, alpha=1e-4, b1=0.9, b2=0.999, eps=1e-8):
    """Chainer AdamRule on fresh state after t identical-gradient steps is not what we test; one step."""
    g = (g * np.float32(scale)).astype(np.float32)
    m = (np.float32(1 - b1) * g).astype(np.float32)
    v = (np.float32(1 - b2) * g * g).astype(np.float32)
    lr = alpha * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)
    return (p - np.float32(lr) * m / (np.sqrt(v) + np.float32(eps))).astype(np.float32)


# 2x64x48 keeps its ids; 1x40x40: uneven weight-gradient splits and 16-pixel tails; 3x24x40: an odd
# batch whose 15- and 60-pixel frames the pixel steps cross (tests/train_layerwise.py CONFIGS)
@pytest.mark.parametrize("shape,frozen", [
    pytest.param((2, 64, 48), False, id="False"), pytest.param((2, 64, 48), True, id="True"),
    pytest.param((1, 40, 40), False, id="1x40x40-False"), pytest.param((1, 40, 40), True, id="1x40x40-True"),
    pytest.param((3, 24, 40), False, id="3x24x40-False"), pytest.param((3, 24, 40), True, id="3x24x40-True")])
def test_train_step_vs_torch_float64(shape, frozen):
    lib = pkg_module("_lib")
    W0 = pkg_module("weights").random_weights(seed=7)
    n, h, w = shape
    x, pt, ht, ig = _data(n, h, w, 3)
    ctx = lib.TrainContext(n, h, w, 0)
    try:
        ctx.set_weights(W0)
        ctx.set_hyper(1e-4)
        names = [t[0] for t in ctx.table]
        # the reference's GradientScaling hook, as its own __call__ applied it per layer
        # (tests/golden/train/host_schedule.json, make_golden_train_host.py)
        mult = _hook_multipliers()
        for nm, sc in mult.items():
            if sc != 1.0:
                ctx.set_grad_scale(names.index(nm), sc)
        vgg = pkg_module("train").VGG_FROZEN
        if frozen:
            for nm in vgg:
                ctx.enable(names.index(nm), False)
        losses = ctx.step(x, pt, ht, ig)
        grads = ctx.get(grads=True)
        W1 = ctx.get()
    finally:
        ctx.close()
    ref_losses, ref_grads = torch_step(W0, x, pt, ht, ig)
    np.testing.assert_allclose(losses, ref_losses, rtol=2e-5)
    worst = 0.0
    for nm in names:
        gW, gb = grads[nm]
        if frozen and nm in vgg:
            assert not gW.any() and not gb.any()
            assert np.array_equal(W1[nm][0], W0[nm][0]) and np.array_equal(W1[nm][1], W0[nm][1])
            continue
        rW, rb = ref_grads[nm]
        sW = max(np.abs(rW).max(), 1e-30)
        errW = np.abs(gW - rW).max() / sW
        errb = np.abs(gb - rb).max() / max(np.abs(rb).max(), 1e-30)
        worst = max(worst, errW, errb)
        assert errW <= 2e-3 and errb <= 2e-3, (nm, errW, errb)
        # the Adam step on the device's own gradients times the reference hook's multiplier
        sc = mult[nm]
        np.testing.assert_allclose(W1[nm][0], adam_ref(W0[nm][0], gW, sc, 1), rtol=0, atol=2e-7)
        np.testing.assert_allclose(W1[nm][1], adam_ref(W0[nm][1], gb, sc, 1), rtol=0, atol=2e-7)
    print("train step: max relative gradient error vs float64 = %.3g" % worst)


def test_updater_schedule_and_loss_decreases():
    T = pkg_module("train")
    up = T.Updater(2, 64, 64, model=pkg_module("weights").random_weights(seed=1))
    rng = np.random.default_rng(0)
    batch = T.synthetic_batch(rng, 2, 64, 64)
    first = up.update(batch)[0]
    for _ in range(5):
        last = up.update(batch)[0]
    assert up.iteration == 6 and last < first  # the same batch: Adam must make progress
    g = up.grads()
    assert not g["conv1_1"][0].any() and g["conv4_3_CPM"][0].any()  # VGG frozen until iteration 2000
    up.ctx.close()


@pytest.mark.parametrize("case", ["posenet_2x48x48", "posenet_1x64x80"])
def test_train_step_losses_vs_reference_compute_loss(case):
    """op_train_step's twelve per-stage losses against the REFERENCE's own compute_loss
    (train_coco_pose_estimation.py:41-73, tests/golden/train/, made by make_golden_train.py) on the
    reference network's own stage outputs for the same weights (seed 0) and input.  The device
    recomputes the forward itself (exact f32), so the losses agree to the forward's 1e-3-level map
    agreement, far tighter in relative terms: rtol 1e-4."""
    from test_train_golden import load_train_case
    from test_forward_golden import case_weights, load_case
    lib = pkg_module("_lib")
    g, _ = load_train_case(case)
    _, d = load_case(case)
    n, h, w = d["x"].shape[0], d["x"].shape[2], d["x"].shape[3]
    ctx = lib.TrainContext(n, h, w, 0)
    try:
        ctx.set_weights(case_weights("posenet", 0))
        losses = ctx.step(d["x"], g["pafs_t"], g["heatmaps_t"], g["ignore_mask"])
    finally:
        ctx.close()
    want = np.stack([g["paf_loss"], g["heat_loss"]], 1).reshape(-1)  # [paf, heat] per stage
    print(case, "max rel loss error vs reference compute_loss: %.3g" % float(np.max(np.abs(losses - want) / want)))
    np.testing.assert_allclose(losses, want, rtol=1e-4)


def adam_step_float64(p, g, m, v, scale, t, alpha=1e-4, b1=0.9, b2=0.999, eps=1e-8, defect=None):
    """Chainer's AdamRule.update_core (eta 1, no weight decay) behind the GradientScaling hook, in
    float64; t = the rule's step count after its increment.  -> (p, m, v, update).  defect: one of the
    mistakes the tolerance of test_adam_step_from_random_moments has to catch."""
    g = g.astype(np.float64) * float(np.float32(scale))
    m1 = m + (1.0 - b1) * (g - m)
    v1 = v + (1.0 - (b1 if defect == "beta1_for_v" else b2)) * (g * g - v)
    tt = t - 1 if defect == "t_off_by_one" else t
    alpha_t = alpha if defect == "no_bias_correction" else alpha * np.sqrt(1.0 - b2 ** tt) / (1.0 - b1 ** tt)
    upd = alpha_t * m1 / (np.sqrt(v1) + eps)
    return p - upd, m1, v1, upd


@pytest.mark.parametrize("t", [1, 7, 1000])
def test_adam_step_from_random_moments(t):
    """Adam away from its degenerate first step (zero moments: the update is alpha sign(g) whatever
    beta1, beta2 and the bias correction are): every layer's m and v set to seeded random values of the
    size of its gradient and its step count to t, one step, then W, b and their m, v against
    adam_step_float64 on the device's own gradient.

    p: atol = 4 * 2^-24 * max(|p|, |alpha_t m / (sqrt(v) + eps)|) with the new m, v (the update).
    m, v: tr_adam works in double and rounds each result to f32 once, so 2^-24 |m'| (|v'|) plus the
    double arithmetic's own error, 2^-50 (|m| + |g|) (v + g^2), which counts only where m' cancels.

    What this test found.  tr_adam used to work in f32: thirteen roundings on the way to p (g scale,
    g - m, its product, m'; g^2, g^2 - v, its product, v'; sqrt, + eps, lr m', the quotient, p - update),
    lr and eps rounded to f32, and 1 - beta taken as 1.0f - (float)beta, which is 1.3e-5 off 0.001 for
    beta2.  With that arithmetic (redone in NumPy) p missed this tolerance at 7 768 - 37 129 of the
    52 311 446 parameters by up to 58 x and v was off by up to 45 roundings at 3.1 million.  With only
    the coefficients mended, measured on an MI355X, p still missed at 63 / 55 / 380 elements (t = 1 / 7 /
    1000) by up to 2.4 / 3.1 / 15.5 x: where |update| >= |p| (parameters within ~1e-4 of zero) the
    tolerance is relative to the update, whose f32 roundings alone reach ~7 * 2^-24, and where
    m' = 0.9 m + 0.1 g cancels the error of m' is large against m' itself.  In double, p is off by its
    one final rounding (at most 2^-24 (|p| + |update|), half the tolerance)."""
    lib = pkg_module("_lib")
    W0 = pkg_module("weights").random_weights(seed=7)
    n, h, w = 1, 16, 16
    batch = _data(n, h, w, 3)
    mult = _hook_multipliers()
    b1, b2 = 0.9, 0.999
    ctx = lib.TrainContext(n, h, w, 0)
    try:
        names = [row[0] for row in ctx.table]
        for nm, sc in mult.items():
            if sc != 1.0:
                ctx.set_grad_scale(names.index(nm), sc)
        ctx.set_hyper(1e-4, b1, b2, 1e-8)
        ctx.set_weights(W0)
        ctx.step(*batch)  # the gradients of W0 (they do not depend on the optimizer state)
        g0 = ctx.get(grads=True)
        rng = np.random.default_rng(100 + t)
        state = {}
        for nm in names:
            st = {"t": t}
            for key, g in (("W", g0[nm][0]), ("b", g0[nm][1])):
                s = max(float(np.sqrt(np.mean(np.square(g.astype(np.float64))))) * mult[nm], 1e-12)
                st["m" + key] = (s * rng.standard_normal(g.shape)).astype(np.float32)
                st["v" + key] = (s * s * rng.uniform(0.0, 1.0, g.shape)).astype(np.float32)
            state[nm] = st
        ctx.set_weights(W0)  # zeroes the state
        ctx.set_state(state)
        ctx.step(*batch)
        g1, W1, S1 = ctx.get(grads=True), ctx.get(), ctx.get_state()
    finally:
        ctx.close()
    u = 2.0 ** -24
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    over = {"p": 0, "m": 0, "v": 0}
    total = 0
    caught = {"beta1_for_v": 0.0, "t_off_by_one": 0.0, "no_bias_correction": 0.0}
    for nm in names:
        assert S1[nm]["t"] == t + 1
        for k, key in ((0, "W"), (1, "b")):
            assert np.array_equal(g1[nm][k], g0[nm][k]), nm  # the same batch and weights: the same gradient
            p0 = W0[nm][k].astype(np.float64)
            m0, v0 = state[nm]["m" + key].astype(np.float64), state[nm]["v" + key].astype(np.float64)
            p, m, v, upd = adam_step_float64(p0, g1[nm][k], m0, v0, mult[nm], t + 1)
            g = g1[nm][k].astype(np.float64) * mult[nm]
            tol_p = 4.0 * u * np.maximum(np.abs(p0), np.abs(upd))
            tiny = 2.0 ** -50
            tol_m = u * np.abs(m) + tiny * (np.abs(m0) + np.abs(g)) + 2.0 ** -149
            tol_v = u * np.abs(v) + tiny * (v0 + g * g) + 2.0 ** -149
            for what, got, want, tol in (("p", W1[nm][k], p, tol_p), ("m", S1[nm]["m" + key], m, tol_m),
                                         ("v", S1[nm]["v" + key], v, tol_v)):
                r = np.abs(got.astype(np.float64) - want) / np.maximum(tol, 1e-300)
                worst[what] = max(worst[what], float(r.max()))
                over[what] += int((r > 1.0).sum())
            total += p0.size
            if nm in ("conv1_1", "conv4_2", "Mconv7_stage6_L2"):  # CPU side: what the tolerance catches
                for defect in caught:
                    bad = adam_step_float64(p0, g1[nm][k], m0, v0, mult[nm], t + 1, defect=defect)[0]
                    caught[defect] = max(caught[defect], float((np.abs(bad - p) / np.maximum(tol_p, 1e-300)).max()))
    print("ADAM t %d: worst err/tol p %.3f m %.3f v %.3f, over the tolerance %s of %d; defect / tolerance %s" % (
        t, worst["p"], worst["m"], worst["v"], over, total, {k: round(v, 1) for k, v in caught.items()}))
    assert all(v > 4.0 for v in caught.values()), caught
    assert not any(over.values()), (over, worst)
