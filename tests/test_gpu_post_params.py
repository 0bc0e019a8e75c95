"""The HIP post-process at NON-DEFAULT run-time parameters, bit for bit against fixtures the
reference's own code made (tests/golden/params/, make_golden_params.py; tests/params_cases.py lists
the sets and what each reaches in the kernels): the standalone calls on full-size maps, the fused
single-scale path, the staged path (eager and graph), the precise path's parameters against the
oracle, and the parameter values the library refuses on the host."""
import numpy as np
import pytest

import params_cases as PC
from oracle import postproc as P
from oracle import precise as PR

pytestmark = pytest.mark.gpu
FWD_TOL = 1e-3  # the project's forward tolerance (test_gpu_parity.py)


def _params(set_name, **more):
    return dict(P.PARAMS, **dict(PC.ALL_SETS[set_name], **more))


@pytest.fixture(scope="module")
def contexts(lib):
    """get(set, weights=None): the one live Context of a parameter set (the previous set's is closed)."""
    live = {}

    def get(set_name, weights=None):
        if set_name not in live:
            for c in live.values():
                c.close()
            live.clear()
            limits = lib.OpLimits()
            if set_name in PC.NOISE_SETS:  # noise_crowd stays in the batched buffers where it can
                limits.max_peaks_per_joint = 2048
            live[set_name] = lib.Context(0, lib.params_from_dict(_params(set_name)), limits)
        if weights is not None:
            live[set_name].set_weights(weights)
        return live[set_name]

    yield get
    for c in live.values():
        c.close()


@pytest.mark.parametrize("set_name,case", PC.pairs())
def test_standalone_calls_vs_reference(contexts, set_name, case):
    """compute_peaks / compute_connections / grouping on full-size maps: heat_fused<HeatFull>,
    limb_pairs_full, limb_greedy, grouping."""
    ctx = contexts(set_name)
    d = PC.load_fixture(set_name, case)
    paf_low, heat_low, _, _ = PC.load_inputs(case)
    mh, mw = int(d["map_h"]), int(d["map_w"])
    peaks = ctx.compute_peaks(P.resize_images(heat_low, mh, mw))
    assert np.array_equal(peaks.reshape(-1, 5), d["all_peaks"])
    if int(d["status"]) == 1:
        return
    conns = ctx.compute_connections(P.resize_images(paf_low, mh, mw), peaks, mw)
    assert np.array_equal(np.concatenate(conns), d["conn"])
    assert np.array_equal(np.cumsum([0] + [len(c) for c in conns]), d["conn_off"])
    if int(d["status"]) == 4:
        with pytest.raises(IndexError):
            ctx.grouping(conns, peaks)
        return
    assert np.array_equal(ctx.grouping(conns, peaks), d["subsets"])


def _check_result(d, call):
    """A (poses, scores, res) call against a fixture; status 1 and 4 as the reference gives them."""
    if int(d["status"]) == 4:
        with pytest.raises(IndexError):
            call()
        return
    poses, scores, res = call()
    assert res.n_peaks == len(d["all_peaks"])
    if int(d["status"]) == 1:
        assert res.n_persons == 0
        return
    assert (res.map_h, res.map_w) == (int(d["map_h"]), int(d["map_w"]))
    assert res.n_persons == int(d["poses_shape"][0])
    assert np.array_equal(poses.reshape(d["poses"].shape), d["poses"])
    assert np.array_equal(scores, d["scores"])


@pytest.mark.parametrize("set_name,case", PC.pairs())
def test_fused_postprocess_vs_reference(contexts, set_name, case):
    """postprocess() from the network maps: heat_fused<HeatLow> and limb_pairs_low with its tables."""
    ctx = contexts(set_name)
    paf_low, heat_low, oh, ow = PC.load_inputs(case)
    _check_result(PC.load_fixture(set_name, case), lambda: ctx.postprocess(paf_low, heat_low, oh, ow))


def _staged_pair(set_name):
    """Two different cases of one frame size per set; the synthetic pair for the `default` set."""
    return ("coincident", "border") if set_name == "default" else ("six_people", "neckless_merge")


@pytest.mark.parametrize("set_name", list(PC.ALL_SETS))
def test_staged_run_vs_reference(contexts, rand_weights, set_name):
    """A 2-frame staged run on staged maps, eager and as a replayed graph."""
    ctx = contexts(set_name, rand_weights)
    cases = _staged_pair(set_name)
    inputs = [PC.load_inputs(c) for c in cases]
    assert inputs[0][2:] == inputs[1][2:] and cases[0] != cases[1]
    maps = np.stack([np.concatenate([paf, heat]) for paf, heat, _, _ in inputs])
    ctx.stage_frames(np.zeros((2, inputs[0][2], inputs[0][3], 3), np.uint8))
    ctx.stage_maps(maps)
    ctx.use_staged_maps(True)
    try:
        for graph in (False, True, True):
            ctx.run_staged(graph=graph)
            ctx.synchronize()
            for i, c in enumerate(cases):
                _check_result(PC.load_fixture(set_name, c), lambda: ctx.fetch_result(i))
    finally:
        ctx.use_staged_maps(False)


# ---- the precise path's parameters (no reference run: cv2 / chainer are absent), vs the oracle ----
SCALES = [[1.0], [0.75, 1.25], [0.5, 1, 1.5]]
# The random network's maps give a few weak connections and hardly a subset of three joints: with
# n_subset_limbs_thresh = 2 and subset_score_thresh = 0.02 single connections are persons (1 .. 6 per
# frame on the oracle's maps), so poses and scores (the line integrals' sums) depend on
# n_integ_points for every scale list (asserted below).
PRECISE_PARAMS = dict(P.PARAMS, inference_img_size=32, n_integ_points=7, n_integ_points_thresh=5,
                      n_subset_limbs_thresh=2, subset_score_thresh=0.02)


@pytest.fixture(scope="module", params=SCALES, ids=lambda s: "scales_" + "_".join(str(v) for v in s))
def precise(request, lib, rand_weights_small):
    """Two 40 x 56 frames through detect_precise, then both through run_staged_precise, with
    n_scales = 1, 2, 3 and n_integ_points = 7: what the device returned, for the tests below."""
    params = dict(PRECISE_PARAMS, inference_scales=request.param)
    for rw, rh, pw, ph in PR.scale_sizes(40, 56, params):
        assert pw >= 16 and ph >= 16  # precise_run refuses a smaller network input
    limits = lib.OpLimits()
    limits.max_peaks_per_joint = 2048
    frames = np.random.default_rng(5).integers(0, 256, (2, 40, 56, 3), dtype=np.uint8)
    c = lib.Context(0, lib.params_from_dict(params), limits)
    try:
        c.set_weights(rand_weights_small)
        c.set_batch_invariant(True)
        single = []
        for f in frames:
            try:
                poses, scores, res, pafs, heat = c.detect_precise(f, return_maps=True)
                single.append({"poses": poses, "scores": scores, "n_peaks": res.n_peaks, "pafs": pafs,
                               "heat": heat, "raised": False})
            except IndexError as e:  # then the oracle raises on these maps too (checked below)
                single.append({"pafs": e.maps[0], "heat": e.maps[1], "raised": True})
        c.stage_frames(frames)
        c.run_staged_precise()
        c.synchronize()
        staged = []
        for i in range(2):
            try:
                poses, scores, res = c.fetch_result(i)
                staged.append({"poses": poses, "scores": scores, "n_peaks": res.n_peaks, "raised": False,
                               "map": (res.map_h, res.map_w)})
            except IndexError:
                staged.append({"raised": True})
        staged_maps = c.fetch_maps(0, 2)
    finally:
        c.close()
    return {"params": params, "frames": frames, "single": single, "staged": staged, "staged_maps": staged_maps}


def test_precise_maps_vs_oracle(precise, rand_weights_small):
    """The mean over n_scales scales (CubicMeanArgs: the sum of ns terms divided by ns)."""
    for f, s in zip(precise["frames"], precise["single"]):
        want_paf, want_heat = PR.precise_maps(rand_weights_small, f, precise["params"])
        assert s["pafs"].shape == want_paf.shape and s["heat"].shape == want_heat.shape
        err = max(float(np.abs(s["pafs"] - want_paf).max()), float(np.abs(s["heat"] - want_heat).max()))
        print("precise maps, scales %s: max|gpu - oracle| = %.3g" % (precise["params"]["inference_scales"], err))
        assert err <= FWD_TOL


def test_precise_postprocess_of_own_maps_vs_oracle(precise):
    seen = False  # some frame's result must depend on n_integ_points = 7
    for f, s in zip(precise["frames"], precise["single"]):
        if s["raised"]:
            with pytest.raises(IndexError):
                PR.postprocess_full(s["pafs"], s["heat"], f.shape[1], precise["params"])
            continue
        wp, ws = PR.postprocess_full(s["pafs"], s["heat"], f.shape[1], precise["params"])
        assert s["n_peaks"] == len(P.compute_peaks_from_heatmaps(s["heat"], precise["params"]))
        assert np.array_equal(s["poses"].reshape(wp.shape), wp) and np.array_equal(s["scores"], ws)
        assert len(ws) >= 1  # a person: the comparison above is not one of empty arrays
        at_default = dict(precise["params"], n_integ_points=P.PARAMS["n_integ_points"],
                          n_integ_points_thresh=P.PARAMS["n_integ_points_thresh"])
        try:
            seen |= not np.array_equal(PR.postprocess_full(s["pafs"], s["heat"], f.shape[1], at_default)[1], ws)
        except IndexError:
            seen = True
    assert seen


def test_staged_precise_equals_per_frame(precise):
    pafs, heat = precise["staged_maps"]
    for i, (s, g) in enumerate(zip(precise["single"], precise["staged"])):
        assert np.array_equal(pafs[i], s["pafs"]) and np.array_equal(heat[i], s["heat"])
        assert g["raised"] == s["raised"]
        if not g["raised"]:
            assert g["map"] == (40, 56) and g["n_peaks"] == s["n_peaks"]
            assert np.array_equal(g["poses"], s["poses"]) and np.array_equal(g["scores"], s["scores"])


# ---- values the library refuses on the host, before any launch ----
@pytest.mark.parametrize("n", [1, 17])
def test_n_integ_points_outside_2_16_refused_at_create(lib, n):
    """op_create checks 2 <= n_integ_points <= 16 (limb_pairs_body's inner[16]) before it touches the
    device."""
    with pytest.raises(ValueError, match="n_integ_points"):
        lib.Context(0, lib.params_from_dict(dict(P.PARAMS, n_integ_points=n)), lib.OpLimits())
    assert lib.last_error()


def _golden(case):
    return dict(np.load(PC.GOLDEN + "/" + case + ".npz"))


def test_gaussian_radius_above_kmaxr_refused(lib):
    """gaussian_sigma 4.5 -> radius 18 > kMaxR: check_shape refuses every post-process call ahead of
    its first launch; the context closes cleanly."""
    d = _golden("one_person")
    c = lib.Context(0, lib.params_from_dict(dict(P.PARAMS, gaussian_sigma=4.5)), lib.OpLimits())
    try:
        with pytest.raises(ValueError, match="outside kernel limits"):
            c.compute_peaks(P.resize_images(d["heat_low"], 320, 320))
        assert lib.last_error()
        with pytest.raises(ValueError, match="outside kernel limits"):
            c.postprocess(d["paf_low"], d["heat_low"], int(d["orig_h"]), int(d["orig_w"]))
    finally:
        c.close()


def test_map_not_above_the_radius_refused(lib):
    """heatmap_size 8 -> an 8 x 8 map, not above the Gaussian radius 10 (one reflection would not
    suffice): refused ahead of the first launch, and the context stays usable for maps it supports."""
    d = _golden("one_person")
    c = lib.Context(0, lib.params_from_dict(dict(P.PARAMS, heatmap_size=8)), lib.OpLimits())
    try:
        with pytest.raises(ValueError, match="outside kernel limits"):
            c.postprocess(d["paf_low"], d["heat_low"], int(d["orig_h"]), int(d["orig_w"]))
        assert lib.last_error()
        with pytest.raises(ValueError, match="outside kernel limits"):
            c.compute_peaks(np.zeros((19, 8, 8), np.float32))
        peaks = c.compute_peaks(P.resize_images(d["heat_low"], int(d["map_h"]), int(d["map_w"])))
        assert np.array_equal(peaks.reshape(-1, 5), d["all_peaks"])
    finally:
        c.close()
