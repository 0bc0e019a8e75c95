"""The GPU-branch peak fixtures (tests/golden/gpu_branch/, made by make_golden_gpu_branch.py from the
reference's own ``else:`` branch, pose_detector.py:111-132, and its own later stages), on the CPU:
the oracle's restatement against them bit for bit, the emulation of the device's separable
arithmetic against them, and the kernel sums that make the tile early-out need a factor.

Measured here (test_device_arithmetic_finds_the_fixture_peaks prints it per set): the largest
|separable - fixture score| / map maximum over every fixture is 9.31e-8 (at sigma 2.5, ksize 3; two f32 roundings against one),
under a third of the 1e-6 the GPU tests allow on scores (tests/test_gpu_peak_mode.py SCORE_RTOL) and 50
times below the fixtures' smallest decision margin (gpu_branch_cases.MARGIN_FLOOR = 5e-6)."""
import functools
import os

import numpy as np
import pytest

import gpu_branch_cases as GC
import params_cases as PC
from oracle import postproc as P


def _params(set_name, case):
    return dict(P.PARAMS, **GC.overrides(set_name, case))


@functools.lru_cache(maxsize=None)
def _heatmaps(case, heatmap_size):
    """The case's upsampled heat maps (19, mh, mw), once per map size."""
    from oracle import cvresize
    _, heat_low, oh, ow = GC.load_inputs(case)
    mw, mh = cvresize.compute_optimal_size(oh, ow, heatmap_size)
    return P.resize_images(heat_low, mh, mw)


def test_fixture_set_is_complete_and_small():
    want = sorted(["%s__%s.npz" % p for p in GC.pairs()] + ["inputs__%s.npz" % c for c in GC.OWN_INPUTS])
    assert sorted(os.listdir(GC.DIR)) == want
    for f in want:
        assert os.path.getsize(os.path.join(GC.DIR, f)) < 64 * 1024, f
    assert GC.KFT == PC.kernel_constant("kFT")
    for s, c in GC.pairs():
        d = GC.load_fixture(s, c)
        assert PC.overrides_of(d) == GC.overrides(s, c) and str(d["input"]) == c
    # the radii: 8 is the compile-time instantiation, the rest reach the run-time one up to kMaxR
    assert sorted({k // 2 for _, k in GC.SETS.values()}) == [1, 2, 3, 4, 8, PC.kernel_constant("kMaxR")]


@pytest.mark.parametrize("set_name,case", GC.pairs())
def test_restatement_equals_the_reference(set_name, case):
    """oracle.postproc's GPU branch gives the reference's peaks, poses and scores bit for bit."""
    d = GC.load_fixture(set_name, case)
    paf_low, heat_low, oh, ow = GC.load_inputs(case)
    prm = _params(set_name, case)
    poses, scores, dbg = P.postprocess(paf_low, heat_low, oh, ow, prm, return_debug=True, branch="gpu")
    assert np.array_equal(np.asarray(dbg["all_peaks"]).reshape(-1, 5), d["all_peaks"])
    assert int(d["status"]) == 0
    assert np.array_equal(np.asarray(poses, np.float64).reshape(d["poses"].shape), d["poses"])
    assert np.array_equal(scores, d["scores"])


def test_properties_the_inputs_exist_for():
    """What the generator asserted on the reference's output, re-read from the committed files."""
    thresh = np.float32(P.PARAMS["heatmap_peak_thresh"])
    for s in GC.CASES["subthresh"]:
        _, heat_low, _, _ = GC.load_inputs("subthresh")
        assert float(heat_low[:-1].max()) < float(thresh) * (1 - 1e-4)
        assert len(GC.load_fixture(s, "subthresh")["all_peaks"]) == 1
    for s in GC.CASES["border"]:
        d = GC.load_fixture(s, "border")
        x, y, mw, mh = d["all_peaks"][:, 1], d["all_peaks"][:, 2], int(d["map_w"]), int(d["map_h"])
        assert np.any(x <= 2) and np.any(x >= mw - 3) and np.any(y <= 2) and np.any(y >= mh - 3)
    for s in GC.CASES["seam"]:
        d = GC.load_fixture(s, "seam")
        assert int(d["map_w"]) >= 2 * GC.KFT and int(d["map_h"]) >= 2 * GC.KFT
        for v in (d["all_peaks"][:, 1], d["all_peaks"][:, 2]):
            assert np.any(v % GC.KFT == GC.KFT - 1) and np.any((v % GC.KFT == 0) & (v > 0))
        assert int(d["poses_shape"][0]) == 1 and int((d["poses"][0, :, 2] > 0).sum()) == len(d["all_peaks"])


@pytest.mark.parametrize("set_name", GC.EVERY_SET)
def test_device_arithmetic_finds_the_fixture_peaks(set_name):
    """separable_like_the_device (two f64 passes, f32 between them: what heat_fused<.., G> computes) on
    every fixture input of the set: the same (joint, x, y) as the reference, its scores within the
    rounding of one extra f32 store.  Largest value over all sets: see the module docstring."""
    sigma, ksize = GC.SETS[set_name]
    worst = 0.0
    for s, case in GC.pairs():
        if s != set_name:
            continue
        d = GC.load_fixture(s, case)
        prm = _params(s, case)
        b = GC.separable_like_the_device(_heatmaps(case, prm["heatmap_size"])[:-1], sigma, ksize)
        nb = np.zeros((4,) + b.shape, np.float32)
        nb[0][:, 1:, :] = b[:, :-1, :]
        nb[1][:, :-1, :] = b[:, 1:, :]
        nb[2][:, :, 1:] = b[:, :, :-1]
        nb[3][:, :, :-1] = b[:, :, 1:]
        got = np.argwhere((b > np.float32(prm["heatmap_peak_thresh"])) & np.all(b[None] >= nb, axis=0))
        pk = d["all_peaks"]
        assert np.array_equal(got[:, [0, 2, 1]].astype(np.float64), pk[:, :3]), (s, case)
        score = b[pk[:, 0].astype(int), pk[:, 2].astype(int), pk[:, 1].astype(int)].astype(np.float64)
        worst = max(worst, float(np.abs(score - pk[:, 3]).max()) / float(b.max()))
    print("%s: max |separable - fixture score| / map maximum = %.3g" % (set_name, worst))
    # three roundings to f32 (the vertical pass's values, the horizontal sum, the fixture's own), each
    # at most 2^-24 of a value no larger than the map maximum: 3 * 2^-24 = 1.8e-7
    assert worst <= 2e-7


def test_tap_sum_table():
    """The reference's kernel is not normalised.  Truncated at 3.2 sigma or more it sums to less than
    1; at sigma <= 0.7 the samples of the density overshoot its integral and it sums to MORE, so a
    filtered value can exceed every source value: heat_fused's tile early-out (postproc.hip
    may_reach) scales the source maximum by max(1, sum) in GPU-branch mode."""
    s = {k: GC.tap_sum_2d(*v) for k, v in GC.SETS.items()}
    print({k: round(v, 5) for k, v in s.items()})
    for k in ("s05_k3", "s05_k5", "s07_k7"):
        assert s[k] > 1 + 1e-4, (k, s[k])
    for k in ("s25_k3", "s25_k5", "s25_k9", "s25_k17", "s25_k33", "s10_k9"):
        assert s[k] < 1, (k, s[k])
    assert abs(s["s05_k5"] - 1.02897) < 1e-5 and abs(s["s25_k17"] - 0.99876) < 1e-5
    # ... and it is the sum of the kernel the reference builds
    for k, (sigma, ksize) in GC.SETS.items():
        ref_sum = float(P.create_gaussian_kernel(sigma, ksize).astype(np.float64).sum())
        assert abs(ref_sum - s[k]) < 1e-6 * s[k], k
