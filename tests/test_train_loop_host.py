"""Validation passes and snapshot / resume of the training loop, host side (no GPU): train.Validator
(the reference's Validator.evaluate + DictSummary.compute_mean, train_coco_pose_estimation.py:
129-159), Updater.save_snapshot / load_snapshot (extensions.snapshot() / --resume FILE, :255,
:265-266), the schedule across a resume and the CLI's validation points, over a fake device context
that records what is asked of it."""
import json
import os

import numpy as np
import pytest

from conftest import pkg_module
from test_train_host import FakeTrainContext


class FakeEvalContext(FakeTrainContext):
    """FakeTrainContext + eval / get / get_state / set_state.  eval's losses depend on the batch (its
    frame count and first target value), so a mean over batches is told from any other combination;
    weights and state are small stand-ins (the host side does not look at their shapes)."""

    def __init__(self, n=2):
        super(FakeEvalContext, self).__init__()
        self.n = n
        self.calls = []
        rng = np.random.default_rng(5)
        self.W = {t[0]: (rng.standard_normal((2, 3)).astype(np.float32), rng.standard_normal(2).astype(np.float32))
                  for t in self.table}
        self.state = {t[0]: dict(mW=rng.standard_normal((2, 3)).astype(np.float32),
                                 vW=rng.random((2, 3)).astype(np.float32),
                                 mb=rng.standard_normal(2).astype(np.float32), vb=rng.random(2).astype(np.float32),
                                 t=int(i % 5)) for i, t in enumerate(self.table)}

    def set_weights(self, w):
        self.calls.append("set_weights")
        if not w:  # (the stand-in model of the updaters built here: the fake keeps its own)
            return
        self.W = {k: (np.array(v[0]), np.array(v[1])) for k, v in w.items()}
        for s in self.state.values():  # as the device: the Adam state is zeroed
            for key in ("mW", "vW", "mb", "vb"):
                s[key] = np.zeros_like(s[key])
            s["t"] = 0

    def set_hyper(self, alpha, beta1=0.9, beta2=0.999, eps=1e-8):
        self.calls.append("set_hyper")
        super(FakeEvalContext, self).set_hyper(alpha, beta1, beta2, eps)

    def enable(self, i, on=True):
        self.calls.append("enable")
        super(FakeEvalContext, self).enable(i, on)

    def step(self, x, pt, ht, ig):
        self.calls.append("step")
        return super(FakeEvalContext, self).step(x, pt, ht, ig)

    def eval(self, x, pt, ht, ig):
        self.calls.append("eval")
        assert x.shape[0] <= self.n and x.dtype == np.float32 and x.shape[1] == 3  # preprocessed, NCHW
        base = float(pt.reshape(-1)[0]) + x.shape[0]
        return base * np.arange(1, 13, dtype=np.float64)

    def get(self, grads=False):
        return {k: (W.copy(), b.copy()) for k, (W, b) in self.W.items()}

    def get_state(self):
        return {k: dict((key, v.copy() if key != "t" else v) for key, v in s.items()) for k, s in self.state.items()}

    def set_state(self, state):
        self.calls.append("set_state")
        self.state = {k: dict(mW=np.array(s["mW"]), vW=np.array(s["vW"]), mb=np.array(s["mb"]), vb=np.array(s["vb"]),
                              t=int(s["t"])) for k, s in state.items()}


def _updater(n=2, resume=False):
    T = pkg_module("train")
    ctx = FakeEvalContext(n)
    return T, ctx, T.Updater(n, 16, 16, model={}, ctx=ctx, resume=resume)


def _batch(m, first):
    pt = np.zeros((m, 38, 2, 2), np.float32)
    pt.reshape(-1)[0] = first
    return (np.zeros((m, 16, 16, 3), np.uint8), pt, np.zeros((m, 19, 2, 2), np.float32), np.zeros((m, 2, 2), np.uint8))


def test_validator_is_the_plain_mean_over_batches():
    T, ctx, up = _updater(2)
    up.iteration = 37
    batches = [_batch(2, 0.5), _batch(2, 0.25), _batch(1, 4.0)]
    n_hyper, n_events = len(ctx.hyper), len(ctx.events)
    ctx.calls.clear()
    got = T.Validator(up, batches).evaluate()
    # per batch: losses = base * (1..12); paf = odd positions 1,3,..,11 (sum 36), heat = 2,4,..,12 (sum 42)
    bases = [0.5 + 2, 0.25 + 2, 4.0 + 1]
    want = {"val/paf": sum(36 * b for b in bases) / 3, "val/heat": sum(42 * b for b in bases) / 3,
            "val/loss": sum(78 * b for b in bases) / 3}
    assert set(got) == set(want)
    for k in want:
        assert got[k] == pytest.approx(want[k], rel=1e-12), k
    # a frame-weighted mean (the shorter last batch counting half) would be another number
    assert got["val/loss"] != pytest.approx(78 * (2 * bases[0] + 2 * bases[1] + bases[2]) / 5, rel=1e-6)
    assert ctx.calls == ["eval"] * 3 and ctx.steps == 0
    assert len(ctx.hyper) == n_hyper and len(ctx.events) == n_events and up.iteration == 37


def test_evaluate_returns_what_update_returns():
    T, ctx, up = _updater(2)
    loss, pl, hl = up.evaluate(_batch(2, 1.0))
    assert len(pl) == 6 and len(hl) == 6 and loss == pytest.approx(sum(pl) + sum(hl))
    assert pl == [3.0 * k for k in (1, 3, 5, 7, 9, 11)] and up.iteration == 0


def test_validator_refuses_a_batch_larger_than_the_context():
    T, ctx, up = _updater(2)
    ctx.calls.clear()
    with pytest.raises(ValueError):
        T.Validator(up, [_batch(2, 0.0), _batch(3, 0.0)]).evaluate()
    assert "eval" not in ctx.calls  # refused before anything ran, never split


def _snapshot_keys(names):
    keys = {"updater/iteration", "updater/alpha", "updater/enabled"}
    for n in names:
        keys |= {"updater/model:main/%s/W" % n, "updater/model:main/%s/b" % n, "updater/optimizer:main/%s/t" % n}
        keys |= {"updater/optimizer:main/%s/%s/%s" % (n, p, s) for p in "Wb" for s in "mv"}
    return keys


def test_snapshot_round_trip(tmp_path):
    T, ctx, up = _updater(2)
    up.iteration, up.alpha = 1234, 1e-5
    up.enable_update("conv2_1")
    path = str(tmp_path / "snapshot_iter_1234.npz")
    up.save_snapshot(path)
    assert os.path.exists(path)
    with np.load(path, allow_pickle=False) as z:
        assert set(z.keys()) == _snapshot_keys(up.names)
        assert int(z["updater/iteration"]) == 1234 and float(z["updater/alpha"]) == 1e-5
        en = z["updater/enabled"]
        assert en.dtype == np.uint8 and en.shape == (92,)
        assert [n for n, e in zip(up.names, en) if not e] == [n for n in T.VGG_FROZEN if n != "conv2_1"]
    W0, S0 = ctx.get(), ctx.get_state()
    assert any(s["t"] for s in S0.values())

    T2, ctx2, up2 = _updater(2, resume=True)  # nothing frozen, other weights, zero state
    ctx2.W = {k: (W * 0, b * 0) for k, (W, b) in ctx2.W.items()}
    ctx2.calls.clear()
    up2.load_snapshot(path)
    calls = [c for c in ctx2.calls if c in ("set_weights", "set_state")]
    assert calls == ["set_weights", "set_state"]  # set_weights zeroes the state: it comes first
    assert up2.iteration == 1234 and up2.alpha == 1e-5 and ctx2.hyper[-1][0] == 1e-5
    assert up2.enabled == up.enabled and ctx2.enabled == ctx.enabled
    assert ctx2.scale == ctx.scale  # the hook, applied again
    W1, S1 = ctx2.get(), ctx2.get_state()
    for n in up.names:
        assert np.array_equal(W1[n][0], W0[n][0]) and np.array_equal(W1[n][1], W0[n][1])
        for key in ("mW", "vW", "mb", "vb"):
            assert np.array_equal(S1[n][key], S0[n][key]), (n, key)
        assert S1[n]["t"] == S0[n]["t"]
    # the existing loader reads the model out of the snapshot (--initmodel SNAPSHOT); it walks the
    # package's layer table, which the fake context shares
    Wl = pkg_module("weights").load_npz(path)
    assert all(np.array_equal(Wl[n][0], W0[n][0]) and np.array_equal(Wl[n][1], W0[n][1]) for n in up.names)


def _resume_at(tmp_path, iteration, alpha=1e-4):
    T, ctx, up = _updater(1)
    up.iteration, up.alpha = iteration, alpha
    path = str(tmp_path / ("snapshot_iter_%d.npz" % iteration))
    up.save_snapshot(path)
    T2, ctx2, up2 = _updater(1)
    up2.load_snapshot(path)
    ctx2.events.clear()
    return T2, ctx2, up2


def test_schedule_continues_across_a_resume(tmp_path):
    """The schedule's edges fall where they fall in an uninterrupted run.  update_core tests the
    iteration count before the update (:95-105, pinned by tests/golden/train/host_schedule.json): the
    update that starts with iteration == 2000 re-enables the VGG layers, the one that starts with
    iteration == 100000 lowers alpha.  So from a snapshot saved at 1999 the first update (1999 ->
    2000) changes nothing and the one after it, the update at iteration 2000, enables exactly
    VGG_FROZEN; from one saved at 2000 that is the very next update."""
    batch = _batch(1, 0.0)
    T, ctx, up = _resume_at(tmp_path, 1999)
    assert sorted(n for n, on in ctx.enabled.items() if not on) == sorted(T.VGG_FROZEN)
    up.update(batch)
    assert up.iteration == 2000 and ctx.events == []
    up.update(batch)
    assert ctx.events == [(n, True) for n in T.VGG_FROZEN] and all(ctx.enabled.values()) and all(up.enabled.values())
    T, ctx, up = _resume_at(tmp_path, 2000)
    up.update(batch)
    assert ctx.events == [(n, True) for n in T.VGG_FROZEN] and up.iteration == 2001

    T, ctx, up = _resume_at(tmp_path, 99999)
    up.update(batch)
    assert ctx.hyper[-1][0] == 1e-4 and up.iteration == 100000
    up.update(batch)
    assert ctx.hyper[-1][0] == 1e-5 and up.alpha == 1e-5
    T, ctx, up = _resume_at(tmp_path, 100000)
    up.update(batch)
    assert ctx.hyper[-1][0] == 1e-5
    T, ctx, up = _resume_at(tmp_path, 150000, alpha=1e-5)  # the lowered alpha itself round-trips
    assert ctx.hyper[-1][0] == 1e-5 and up.alpha == 1e-5


def _run_cli(tmp_path, monkeypatch, name, extra):
    T = pkg_module("train")
    monkeypatch.setattr(pkg_module("weights"), "random_weights", lambda seed=0: {})  # nothing to upload
    ctx = FakeEvalContext(2)
    out = str(tmp_path / name)
    assert T.main(["--batchsize", "2", "--insize", "16", "--out", out] + extra, ctx=ctx) == 0
    with open(os.path.join(out, "log")) as f:
        return ctx, out, json.load(f)


def test_cli_validation_points(tmp_path, monkeypatch):
    ctx, out, log = _run_cli(tmp_path, monkeypatch, "val", ["--test", "--iteration", "20", "--log-interval", "1",
                                               "--valbatchsize", "2", "--val_samples", "5"])
    files = sorted(os.listdir(out))
    assert files == ["log", "model_iter_10.npz", "model_iter_20.npz", "snapshot_iter_10.npz", "snapshot_iter_20.npz"]
    assert [e["iteration"] for e in log] == list(range(1, 21))
    assert [e["iteration"] for e in log if "val/loss" in e] == [10, 20]
    assert all("main/loss" in e for e in log)
    assert {"val/loss", "val/paf", "val/heat"} <= set(log[9])
    assert ctx.steps == 20 and ctx.calls.count("eval") == 2 * 3  # 5 samples in batches of 2, 2, 1, twice
    with np.load(os.path.join(out, "snapshot_iter_10.npz"), allow_pickle=False) as z:
        assert int(z["updater/iteration"]) == 10


def test_cli_without_new_flags_logs_what_it_logged(tmp_path, monkeypatch):
    ctx, out, log = _run_cli(tmp_path, monkeypatch, "plain", ["--iteration", "3"])
    assert [sorted(e) for e in log] == [sorted(["iteration", "main/loss", "main/paf", "main/heat", "elapsed_s"])] * 3
    assert sorted(os.listdir(out)) == ["log", "model_iter_3.npz"] and "eval" not in ctx.calls


def test_cli_log_interval_means_and_resume(tmp_path, monkeypatch):
    ctx, out, log = _run_cli(tmp_path, monkeypatch, "first", ["--iteration", "10", "--val-interval", "5", "--log-interval", "4",
                                                 "--valbatchsize", "2", "--val_samples", "2"])
    assert [e["iteration"] for e in log] == [4, 8, 10]  # LogReport entries + the remainder
    assert [("val/loss" in e) for e in log] == [False, True, True]
    ctx2, out2, log2 = _run_cli(tmp_path, monkeypatch, "second", ["--iteration", "2", "--resume-from",
                                                     os.path.join(out, "snapshot_iter_10.npz")])
    assert [e["iteration"] for e in log2] == [11, 12] and os.path.exists(os.path.join(out2, "model_iter_12.npz"))
    assert "set_state" in ctx2.calls
