"""GPU-branch peak semantics (op_set_peak_mode, include/openpose_hip.h) against the reference's GPU
branch (pose_detector.py:38-44, 111-132): against fixtures its own code made under a NumPy-backed
``xp`` with the convolution stood in by the exact sum (tests/golden/gpu_branch/,
make_golden_gpu_branch.py; gpu_branch_cases.py lists the (sigma, ksize) sets and cases), and against
the oracle's restatement (oracle/postproc.py compute_peaks_gpu_branch), which
test_gpu_branch_golden.py holds to the same fixtures bit for bit.

The device filter is separable f64 with one f32 rounding between the passes; the reference's stand-in
and the oracle are the exact 2-D sum rounded once.  Tolerance: peak sets and poses exact (no peak
decision of the golden inputs lies within 5e-7 of a tie relative to the map maximum, asserted below;
none of the fixtures' within 5e-6, asserted by their generator; the two forms differ by at most
9.4e-8, test_gpu_branch_golden.py), scores within 1e-6 relative."""
import numpy as np
import pytest

import gpu_branch_cases as GC
from conftest import golden_cases, load_golden, people_image
from oracle import postproc as P

pytestmark = pytest.mark.gpu
SCORE_RTOL = 1e-6


@pytest.fixture(scope="module")
def gctx(lib, rand_weights):
    c = lib.Context(0)
    c.set_weights(rand_weights)
    c.set_peak_mode("gpu", 17)
    yield c
    c.close()


def _decision_margin(heat_low, orig_h, orig_w, params=P.PARAMS):
    """Relative room a rounding difference has before one peak decision flips: for a peak, its
    smallest gap to the threshold or a neighbour; for any other pixel, its largest failing gap (all
    of them must flip to make it a peak).  Neighbours outside the map count as 0
    (gpu_branch_cases.decision_margin, on the oracle's filtered maps)."""
    from oracle import cvresize
    mw, mh = cvresize.compute_optimal_size(orig_h, orig_w, params["heatmap_size"])
    return GC.decision_margin(P.gpu_branch_filter(P.resize_images(heat_low, mh, mw)[:-1], params),
                              params["heatmap_peak_thresh"])


@pytest.mark.parametrize("case", golden_cases())
def test_gpu_branch_postprocess_vs_oracle(gctx, case):
    d = load_golden(case)
    oh, ow = int(d["orig_h"]), int(d["orig_w"])
    poses, scores, res = gctx.postprocess(d["paf_low"], d["heat_low"], oh, ow)
    want_p, want_s, dbg = P.postprocess(d["paf_low"], d["heat_low"], oh, ow, return_debug=True, branch="gpu")
    # no decision within ~7 f32 ulp of a tie (the golden maps' closest is 7.5e-7, noise_crowd), where
    # the device's two-pass rounding (~1e-7) could flip it
    assert _decision_margin(d["heat_low"], oh, ow) > 5e-7
    assert res.n_peaks == len(dbg["all_peaks"])
    assert res.n_persons == len(want_s)
    if len(want_s):
        assert np.array_equal(poses.reshape(np.asarray(want_p).shape), np.asarray(want_p, np.float64))
        assert np.allclose(scores, want_s, rtol=SCORE_RTOL, atol=0)


def test_peak_mode_round_trip_restores_cpu_branch(lib, rand_weights):
    """Switching to the GPU branch and back gives the reference's CPU-branch golden bit for bit."""
    c = lib.Context(0)
    try:
        c.set_weights(rand_weights)
        d = load_golden("six_people")
        args = (d["paf_low"], d["heat_low"], int(d["orig_h"]), int(d["orig_w"]))
        c.set_peak_mode("gpu")
        _, sg, _ = c.postprocess(*args)
        c.set_peak_mode("cpu")
        p, s, _ = c.postprocess(*args)
        assert np.array_equal(p.reshape(d["poses"].shape), d["poses"]) and np.array_equal(s, d["scores"])
        assert not np.array_equal(sg, s)  # the unnormalised kernel gives other scores
        with pytest.raises(Exception):
            c.set_peak_mode("gpu", 16)  # even ksize
        with pytest.raises(Exception):
            c.set_peak_mode("gpu", 35)  # radius past the tiled kernel's 16
    finally:
        c.close()


@pytest.mark.parametrize("graph", [False, True])
def test_gpu_branch_staged_batch_equals_single(gctx, graph):
    """The batched path (staged maps, eager and hipGraph) gives each frame the single-frame result."""
    cases = ["six_people", "noise_crowd"]
    ds = [load_golden(c) for c in cases]
    oh, ow = int(ds[0]["orig_h"]), int(ds[0]["orig_w"])
    ds = [d for d in ds if (int(d["orig_h"]), int(d["orig_w"])) == (oh, ow) and d["heat_low"].shape == ds[0]["heat_low"].shape]
    maps = np.stack([np.concatenate([d["paf_low"], d["heat_low"]]) for d in ds])
    single = [gctx.postprocess(d["paf_low"], d["heat_low"], oh, ow) for d in ds]
    gctx.stage_frames(np.zeros((len(ds), oh, ow, 3), np.uint8))
    gctx.stage_maps(maps)
    gctx.use_staged_maps(True)
    try:
        for _ in range(2):
            gctx.run_staged(graph=graph)
            gctx.synchronize()
            for i in range(len(ds)):
                p, s, r = gctx.fetch_result(i)
                assert r.n_peaks == single[i][2].n_peaks
                assert np.array_equal(p, single[i][0]) and np.array_equal(s, single[i][1])
    finally:
        gctx.use_staged_maps(False)


# ---- every kernel size and sigma, against the reference's own GPU branch (tests/golden/gpu_branch/) ----
def _params(set_name, case):
    return dict(P.PARAMS, **GC.overrides(set_name, case))


def _context_key(set_name, case):
    prm = _params(set_name, case)
    return prm["gaussian_sigma"], prm["heatmap_size"]


@pytest.fixture(scope="module")
def sigma_contexts(lib, rand_weights):
    """get(set, case): the one live Context of the pair's (gaussian_sigma, heatmap_size), switched to
    the set's ksize (the previous parameters' context is closed)."""
    live = {}

    def get(set_name, case):
        key = _context_key(set_name, case)
        if key not in live:
            for c in live.values():
                c.close()
            live.clear()
            live[key] = lib.Context(0, lib.params_from_dict(_params(set_name, case)), lib.OpLimits())
            live[key].set_weights(rand_weights)
        live[key].set_peak_mode("gpu", GC.SETS[set_name][1])
        return live[key]

    yield get
    for c in live.values():
        c.close()


def _check_fixture(d, out):
    """A (poses, scores, res) result against a fixture of the reference's GPU branch.  The single-scale
    path returns no peak list: the peaks are held by their count and by the keypoint coordinates of
    the poses (every peak of `seam` and most of the others' are part of one)."""
    poses, scores, res = out
    assert int(d["status"]) == 0
    assert (res.map_h, res.map_w) == (int(d["map_h"]), int(d["map_w"]))
    assert res.n_peaks == len(d["all_peaks"])
    assert res.n_persons == len(d["scores"])
    assert np.array_equal(poses.reshape(d["poses"].shape), d["poses"])
    assert np.allclose(scores, d["scores"], rtol=SCORE_RTOL, atol=0)


@pytest.mark.parametrize("set_name,case", sorted(GC.pairs(), key=lambda p: _context_key(*p)))
def test_gpu_branch_postprocess_vs_reference(sigma_contexts, set_name, case):
    """heat_fused<HeatLow, 0, true> at radius 1, 2, 3, 4 and 16 and <HeatLow, 8, true>: zero padding at
    the map border (`border`), peaks on both sides of a tile seam (`seam`), and a tile whose sources
    all lie below the threshold while the kernel, summing to more than 1, lifts one value over it
    (`subthresh`: the early-out of may_reach)."""
    ctx = sigma_contexts(set_name, case)
    paf_low, heat_low, oh, ow = GC.load_inputs(case)
    _check_fixture(GC.load_fixture(set_name, case), ctx.postprocess(paf_low, heat_low, oh, ow))


@pytest.mark.parametrize("set_name", ["s25_k5", "s05_k5"])
def test_gpu_branch_nine_staged_frames(sigma_contexts, set_name):
    """Nine staged frames (more than 8: the XCD-major block order; not a multiple of 8: the blocks of
    the padded grid that leave at f >= n_frames), eager and as a graph replayed twice: each frame
    equals its single-frame result bit for bit, and the reference's fixture."""
    cases = ["six_people", "border", "coincident"]
    ctx = sigma_contexts(set_name, cases[0])
    inputs = {c: GC.load_inputs(c) for c in cases}
    assert len({(i[0].shape, i[2], i[3]) for i in inputs.values()}) == 1
    oh, ow = inputs[cases[0]][2:]
    order = [cases[i % len(cases)] for i in range(9)]
    single = {c: ctx.postprocess(*inputs[c]) for c in cases}
    for c in cases:
        _check_fixture(GC.load_fixture(set_name, c), single[c])
    ctx.stage_frames(np.zeros((len(order), oh, ow, 3), np.uint8))
    ctx.stage_maps(np.stack([np.concatenate(inputs[c][:2]) for c in order]))
    ctx.use_staged_maps(True)
    try:
        for graph in (False, True, True):
            ctx.run_staged(graph=graph)
            ctx.synchronize()
            for i, c in enumerate(order):
                p, s, r = ctx.fetch_result(i)
                assert r.n_peaks == single[c][2].n_peaks
                assert np.array_equal(p, single[c][0]) and np.array_equal(s, single[c][1])
                _check_fixture(GC.load_fixture(set_name, c), (p, s, r))
    finally:
        ctx.use_staged_maps(False)


def test_peak_mode_switches_rewrite_the_taps(lib, rand_weights):
    """gpu/5 -> gpu/17 -> cpu -> gpu/33 -> gpu/3 on one context: every step gives its own fixture (the
    CPU golden, bit for bit, for the cpu step), so the tap table at kGaussGpuOff is rewritten by each
    switch, not appended to or left over from a longer kernel."""
    c = lib.Context(0)
    try:
        c.set_weights(rand_weights)
        args = GC.load_inputs("six_people")
        for mode, ksize in (("gpu", 5), ("gpu", 17), ("cpu", None), ("gpu", 33), ("gpu", 3)):
            c.set_peak_mode(mode, ksize)
            out = c.postprocess(*args)
            if mode == "gpu":
                _check_fixture(GC.load_fixture("s25_k%d" % ksize, "six_people"), out)
            else:
                d = load_golden("six_people")
                assert out[2].n_peaks == len(d["all_peaks"])
                assert np.array_equal(out[0].reshape(d["poses"].shape), d["poses"]) and np.array_equal(out[1], d["scores"])
    finally:
        c.close()


def test_map_not_above_the_gpu_radius_refused(lib):
    """heatmap_size 16 -> a 16 x 16 map, not above the GPU branch's radius 16 at ksize 33: refused by
    check_shape ahead of the first launch (maps no larger than the radius stay unsupported in this
    mode), and the context stays usable: the same map at ksize 5 against the restatement, and a
    96 x 96 map through the standalone peaks."""
    paf_low, heat_low, _, _ = GC.load_inputs("subthresh")
    heat_low = heat_low * np.float32(4)  # the bump well above the threshold
    prm = dict(P.PARAMS, heatmap_size=16)
    c = lib.Context(0, lib.params_from_dict(prm), lib.OpLimits())
    try:
        c.set_peak_mode("gpu", 33)
        with pytest.raises(ValueError, match="outside kernel limits"):
            c.postprocess(paf_low, heat_low, 96, 96)
        assert lib.last_error()
        c.set_peak_mode("gpu", 5)
        p5 = dict(prm, ksize=5)
        assert _decision_margin(heat_low, 96, 96, p5) > GC.MARGIN_FLOOR
        _, _, dbg = P.postprocess(paf_low, heat_low, 96, 96, p5, return_debug=True, branch="gpu")
        _, _, res = c.postprocess(paf_low, heat_low, 96, 96)
        assert (res.map_h, res.map_w) == (16, 16) and res.n_peaks == len(dbg["all_peaks"]) == 1
        c.set_peak_mode("gpu", 33)
        full = P.resize_images(heat_low, 96, 96)
        want = P.compute_peaks_from_heatmaps(full, prm)
        assert len(want) == 1
        assert np.array_equal(c.compute_peaks(full).reshape(-1, 5), np.asarray(want).reshape(-1, 5))
    finally:
        c.close()


def _near_ties(heat_low, orig_h, orig_w, eps=1e-6):
    """Peak decisions within eps (relative to the map maximum) of a tie: the pixels whose decision
    a rounding difference of that size could flip (see _decision_margin)."""
    from oracle import cvresize
    mw, mh = cvresize.compute_optimal_size(orig_h, orig_w, 320)
    f = P.gpu_branch_filter(P.resize_images(heat_low, mh, mw)[:-1]).astype(np.float64)
    pad = np.pad(f, ((0, 0), (1, 1), (1, 1)))
    g = [f - np.float64(np.float32(0.05))]
    for dy, dx in ((0, 1), (2, 1), (1, 0), (1, 2)):
        g.append(f - pad[:, dy:dy + f.shape[1], dx:dx + f.shape[2]])
    g = np.stack(g)
    peak = (g[0] > 0) & np.all(g[1:] >= 0, axis=0)
    m = np.where(peak, np.abs(g).min(axis=0),
                 np.where(np.concatenate([(g[0] <= 0)[None], g[1:] < 0]), np.abs(g), 0.0).max(axis=0))
    return int((m < eps * max(float(f.max()), 1e-30)).sum())


def test_pose_detector_gpu_branch(pkg, rand_weights):
    """PoseDetector(peak_branch='gpu')(img) runs the GPU-branch post-process: equal bit for bit to the
    context's GPU-branch post-process of the same device forward, different from the CPU branch, and
    its peak count within the near-tie decisions of the oracle's (the random network's noise maps
    hold decisions within 1e-7 of a tie, so peaks are compared by count here; the golden cases
    above compare them exactly)."""
    det = pkg.PoseDetector("posenet", model=rand_weights, device=0, peak_branch="gpu")
    img = people_image()
    x = det._ctx.preprocess(img, 368, 368)
    paf, heat = det._ctx.forward(x)
    poses, scores = det(img)
    p2, s2, r2 = det._ctx.postprocess(paf[0], heat[0], img.shape[0], img.shape[1])
    assert np.array_equal(np.asarray(poses, np.float64).reshape(p2.shape), p2) and np.array_equal(scores, s2)
    _, _, dbg = P.postprocess(paf[0], heat[0], img.shape[0], img.shape[1], return_debug=True, branch="gpu")
    _, _, dbg_cpu = P.postprocess(paf[0], heat[0], img.shape[0], img.shape[1], return_debug=True)
    ties = _near_ties(heat[0], img.shape[0], img.shape[1])
    print("GPU-branch peaks: device %d, oracle %d (CPU branch %d), near-tie decisions %d" % (
        r2.n_peaks, len(dbg["all_peaks"]), len(dbg_cpu["all_peaks"]), ties))
    assert abs(r2.n_peaks - len(dbg["all_peaks"])) <= ties
    assert len(dbg["all_peaks"]) != len(dbg_cpu["all_peaks"]) or not np.array_equal(dbg["all_peaks"], dbg_cpu["all_peaks"])


def test_precise_mode_keeps_the_cpu_branch(lib, rand_weights_small):
    """detect_precise takes the CPU branch whatever the peak mode (the reference's precise heatmaps
    are NumPy arrays: pose_detector.py:470-475)."""
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (96, 128, 3), dtype=np.uint8)
    out = []
    for mode in ("cpu", "gpu"):
        c = lib.Context(0)
        try:
            c.set_weights(rand_weights_small)
            c.set_peak_mode(mode)
            p, s, r = c.detect_precise(img)
            out.append((p, s, r.n_peaks))
        finally:
            c.close()
    assert out[0][2] == out[1][2]
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
