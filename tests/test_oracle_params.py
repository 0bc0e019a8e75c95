"""The CPU oracle against the reference's own outputs at NON-DEFAULT parameters
(tests/golden/params/, made by make_golden_params.py), and the conditions the choice of parameter
sets rests on: which kernel branch each set reaches, recomputed from the shapes and the kernels'
constants, so that a later change of either cannot silently empty the coverage."""
import re

import numpy as np
import pytest

import params_cases as PC
from oracle import cvresize, postproc as P


def _params(set_name):
    return dict(P.PARAMS, **PC.ALL_SETS[set_name])


def test_every_fixture_exists_and_records_its_overrides():
    want = sorted(["%s__%s.npz" % p for p in PC.pairs()] + ["inputs__%s.npz" % c for c in PC.SYNTH_CASES])
    assert PC.fixture_files() == want
    for s, c in PC.pairs():
        d = PC.load_fixture(s, c)
        assert PC.overrides_of(d) == PC.ALL_SETS[s]
        assert str(d["input"]) == c
        _, _, oh, ow = PC.load_inputs(c)
        mw, mh = cvresize.compute_optimal_size(oh, ow, _params(s)["heatmap_size"])
        assert (int(d["map_h"]), int(d["map_w"])) == (mh, mw)


@pytest.mark.parametrize("set_name,case", PC.pairs())
def test_oracle_matches_reference(set_name, case):
    d = PC.load_fixture(set_name, case)
    prm = _params(set_name)
    paf_low, heat_low, oh, ow = PC.load_inputs(case)
    mh, mw = int(d["map_h"]), int(d["map_w"])
    pafs = P.resize_images(paf_low, mh, mw)
    heat = P.resize_images(heat_low, mh, mw)
    peaks = P.compute_peaks_from_heatmaps(heat, prm)
    assert np.array_equal(np.asarray(peaks).reshape(-1, 5), d["all_peaks"])
    if int(d["status"]) == 1:
        poses, scores = P.postprocess(paf_low, heat_low, oh, ow, prm)
        assert poses.shape == (0, 18, 3) and scores.shape == (0,)
        return
    conns = P.compute_connections(pafs, peaks, mw, prm)
    assert np.array_equal(np.concatenate(conns), d["conn"])
    assert np.array_equal(np.cumsum([0] + [len(c) for c in conns]), d["conn_off"])
    if int(d["status"]) == 4:
        with pytest.raises(IndexError):
            P.grouping_key_points(conns, peaks, prm)
        return
    subsets = P.grouping_key_points(conns, peaks, prm)
    assert np.array_equal(subsets, d["subsets"])
    poses, scores = P.postprocess(paf_low, heat_low, oh, ow, prm)
    assert tuple(np.asarray(poses).shape) == tuple(d["poses_shape"])
    assert np.array_equal(np.asarray(poses, np.float64).reshape(d["poses"].shape), d["poses"])
    assert np.array_equal(scores, d["scores"])


# ---- each set changes what its parameters feed: a kernel that ignored them cannot pass ----
def _default(case):
    return dict(np.load(PC.GOLDEN + "/" + case + ".npz")) if case in PC.GOLDEN_CASES else \
        PC.load_fixture("default", case)


def _cases_of(set_name, tiled=False):
    return [c for s, c in PC.pairs() if s == set_name and (tiled or c not in PC.TILED_CASES)]


def _same(a, b, key):
    return (key in a) == (key in b) and (key not in a or np.array_equal(a[key], b[key]))


@pytest.mark.parametrize("set_name", PC.STAGE_PEAKS)
def test_set_changes_the_peaks(set_name):
    assert any(not _same(PC.load_fixture(set_name, c), _default(c), "all_peaks") for c in _cases_of(set_name))


@pytest.mark.parametrize("set_name", PC.STAGE_CONNECTIONS)
def test_set_changes_the_connections_alone(set_name):
    """The line integral's parameters leave the peaks as they are and change the connections."""
    for c in _cases_of(set_name):
        assert _same(PC.load_fixture(set_name, c), _default(c), "all_peaks")
    assert any(not _same(PC.load_fixture(set_name, c), _default(c), "conn") for c in _cases_of(set_name))


@pytest.mark.parametrize("set_name", PC.STAGE_PERSONS)
def test_set_changes_the_persons(set_name):
    assert any(not _same(PC.load_fixture(set_name, c), _default(c), "subsets") for c in _cases_of(set_name))
    assert any(len(PC.load_fixture(set_name, c).get("scores", ())) != len(_default(c).get("scores", ()))
               for c in _cases_of(set_name))


def test_every_set_is_classified():
    assert set(PC.STAGE_PEAKS) | set(PC.STAGE_CONNECTIONS) | set(PC.STAGE_PERSONS) == set(PC.SETS)


# A parameter of a set that changes nothing on the set's cases, and the set that holds it instead.
# (`thresh` is kept as first chosen: its subsets' score / joint-count ratios start at 1.27, so 0.45
# drops none of them; `score` overrides that one parameter with a value that does.)
INERT = {("thresh", "subset_score_thresh"): "score"}
_ORDER = list(PC.TILED_CASES) + ["noise_crowd", "twenty_720p", "six_people", "neckless_merge", "one_person",
                                "portrait_four"] + PC.SYNTH_CASES


def _differs_with_default(set_name, name):
    """True when the oracle, run with the set's overrides but `name` put back to its default, gives
    other peaks, connections or subsets than the fixture on at least one of the set's cases."""
    prm = dict(_params(set_name), **{name: P.PARAMS[name]})
    for c in sorted(_cases_of(set_name, tiled=True), key=_ORDER.index):
        d = PC.load_fixture(set_name, c)
        paf_low, heat_low, oh, ow = PC.load_inputs(c)
        try:
            _, _, dbg = P.postprocess(paf_low, heat_low, oh, ow, prm, return_debug=True)
        except IndexError:
            if int(d["status"]) != 4:
                return True
            continue
        if not np.array_equal(np.asarray(dbg["all_peaks"]).reshape(-1, 5), d["all_peaks"]):
            return True
        if dbg["connections"] is not None and not (
                np.array_equal(np.concatenate(dbg["connections"]), d["conn"]) and
                np.array_equal(dbg["subsets"], d["subsets"])):
            return True
    return False


@pytest.mark.parametrize("set_name,name", [(s, k) for s, ov in PC.SETS.items() for k in ov])
def test_each_overridden_parameter_is_discriminated(set_name, name):
    """Per parameter, not per set: a kernel that ignored this ONE parameter (used its default) cannot
    reproduce the set's fixtures."""
    if (set_name, name) in INERT:
        assert not _differs_with_default(set_name, name)  # else the entry is stale: drop it
        assert name in PC.SETS[INERT[(set_name, name)]]
        assert _differs_with_default(INERT[(set_name, name)], name)
        return
    assert _differs_with_default(set_name, name)


def test_kept_subsets_pass_the_grouping_bounds():
    for s in ("thresh", "score"):
        prm = _params(s)
        for c in _cases_of(s, tiled=True):
            sub = PC.load_fixture(s, c)["subsets"]
            assert np.all(sub[:, 19] >= prm["n_subset_limbs_thresh"])
            assert np.all(sub[:, 18] / sub[:, 19] >= prm["subset_score_thresh"])
    dropped = {c: len(_default(c)["subsets"]) - len(PC.load_fixture("score", c)["subsets"]) for c in _cases_of("score")}
    assert dropped["six_people"] >= 1 and dropped["twenty_720p"] >= 2 and dropped["neckless_merge"] >= 3, dropped


# ---- the branch conditions the sets were chosen for ----
def _i0(o, L, oL):
    """axis_tap's source index (postproc.hip): floor of the align-corners coordinate, clamped."""
    u = np.linspace(0.0, L - 1, oL)[o]
    return np.clip(np.floor(u).astype(int), 0, L - 2)


def _reflect(i, L):
    i = np.where(i < 0, -i - 1, i)
    return np.clip(np.where(i >= L, 2 * L - 1 - i, i), 0, L - 1)


def _window_extent(L_low, L_map, radius):
    """Largest low-res window edge heat_fused gathers along one axis over the axis' tiles."""
    kFT = PC.kernel_constant("kFT")
    best = 0
    for y0 in range(0, L_map, kFT):
        hr = min(kFT + 2, L_map + 1 - y0)
        rows = _reflect(np.arange(y0 - 1 - radius, y0 - 1 - radius + hr + 2 * radius), L_map)
        i0 = _i0(rows, L_low, L_map)
        best = max(best, int(i0.max()) + 2 - int(i0.min()))
    return best


def _map_and_low(case, set_name):
    paf_low, _, oh, ow = PC.load_inputs(case)
    mw, mh = cvresize.compute_optimal_size(oh, ow, _params(set_name)["heatmap_size"])
    return paf_low.shape[1], paf_low.shape[2], mh, mw


def _radius(set_name):
    return len(P.gaussian_weights(_params(set_name)["gaussian_sigma"])) // 2


def test_low_res_window_branches():
    """heat_fused stages the low-res window in LDS only where it fits kFW x kFW: at the default and at
    every upsampling set it does; map40 on the two non-square cases takes the unstaged branch."""
    kFW = PC.kernel_constant("kFW")
    for case, unstaged in (("twenty_720p", True), ("portrait_four", True), ("one_person", False)):
        lh, lw, mh, mw = _map_and_low(case, "map40")
        ext = max(_window_extent(lh, mh, _radius("map40")), _window_extent(lw, mw, _radius("map40")))
        assert (ext > kFW) == unstaged, (case, ext)
        assert max(lh, lw) > kFW if unstaged else max(lh, lw) <= kFW
    for set_name in ("integ16", "map184", "sigma1_map248"):
        for case in ("twenty_720p", "portrait_four"):
            lh, lw, mh, mw = _map_and_low(case, set_name)
            r = _radius(set_name)
            assert max(_window_extent(lh, mh, r), _window_extent(lw, mw, r)) <= kFW


def test_tile_counts_and_upsampling_ratios():
    kFT = PC.kernel_constant("kFT")
    tiles = lambda c, s: tuple(-(-v // kFT) for v in _map_and_low(c, s)[2:])  # noqa: E731
    assert tiles("one_person", "map40") == (1, 1) and tiles("twenty_720p", "map40") == (1, 2)
    assert tiles("one_person", "map184") == (3, 3) and tiles("twenty_720p", "map184") == (3, 6)
    assert tiles("portrait_four", "sigma1_map248") == (6, 4)
    lh, lw, mh, mw = _map_and_low("twenty_720p", "map40")
    assert mh < lh and mw < lw  # a true downsample
    lh, lw, mh, mw = _map_and_low("one_person", "map184")
    assert mh == 4 * lh


def test_gaussian_radius_and_map_limits():
    kMaxR = PC.kernel_constant("kMaxR")
    assert _radius("sigma1_map248") == 4 and _radius("map40") == 10  # 10: the register-blocked kernel
    for s in PC.ALL_SETS:
        for c in _cases_of(s):
            _, _, mh, mw = _map_and_low(c, s)
            assert _radius(s) <= kMaxR and min(mh, mw) > _radius(s)
    # the refused values of test_gpu_post_params.py
    assert len(P.gaussian_weights(4.5)) // 2 > kMaxR
    assert cvresize.compute_optimal_size(480, 480, 8)[0] <= _radius("default")


def test_pairwise_sum_branches():
    """limb_pairs_body: n < 8 sequential; else 8 accumulators, a loop body over i = 8 .. n - n % 8 in
    steps of 8, and a tail of n % 8."""
    n = {s: PC.SETS[s]["n_integ_points"] for s in ("integ16", "integ13", "integ7", "integ2")}
    assert n["integ16"] - n["integ16"] % 8 > 8 and n["integ16"] % 8 == 0   # loop body, no tail
    assert n["integ13"] - n["integ13"] % 8 == 8 and n["integ13"] % 8 == 5  # no loop body, tail of 5
    assert 2 < n["integ7"] < 8                                              # sequential
    assert P.PARAMS["n_integ_points"] - P.PARAMS["n_integ_points"] % 8 == 8  # the default: tail of 2 only
    # the kernel's limits (op_create, check_shape): 2 .. 16 = the size of limb_pairs_body's inner[]
    with open(PC.CSRC + "/postproc.hip") as f:
        src = f.read()
    size = int(re.search(r"double\s+inner\s*\[\s*(\d+)\s*\]", src).group(1))
    hi = int(re.search(r"n_integ\s*>\s*(\d+)", src).group(1))
    lo = int(re.search(r"n_integ\s*<\s*(\d+)", src).group(1))
    assert n["integ16"] == hi == size and n["integ2"] == lo == 2


def test_pair_table_branches():
    """limb_pairs_low samples the map directly below kPairsStage candidate pairs of a (frame, limb)
    and through LDS tap tables + PAF planes from there on (launch_post_maps: `tables` 2 where both fit
    64 KiB, as they do for every map here): the fixtures hold limbs on both sides."""
    stage = PC.kernel_constant("kPairsStage")
    limbs = P.PARAMS["limbs_point"]
    for s in PC.NOISE_SETS + ["map40", "sigma1_map248"]:
        sides = set()
        for c in _cases_of(s):
            lh, lw, mh, mw = _map_and_low(c, s)
            assert (mh + mw) * 24 + 2 * lh * lw * 4 <= 64 * 1024  # tables == 2
            cnt = np.bincount(PC.load_fixture(s, c)["all_peaks"][:, 0].astype(int), minlength=18)
            sides |= {bool(cnt[a] * cnt[b] >= stage) for a, b in limbs if cnt[a] * cnt[b] > 0}
        # (`thresh` leaves noise_crowd too few peaks for a staged limb)
        assert (True in sides) == (s in ("integ2", "integ16", "map184")) and False in sides, (s, sides)
    # 92 x 92 network maps: the tap tables alone fit (`tables` 1), for limbs on both sides of the bound
    for s in PC.TILED_SETS:
        for c in PC.TILED_CASES:
            lh, lw, mh, mw = _map_and_low(c, s)
            assert (mh + mw) * 24 + 2 * lh * lw * 4 > 64 * 1024 >= 48 * 1024 >= (mh + mw) * 24
            cnt = np.bincount(PC.load_fixture(s, c)["all_peaks"][:, 0].astype(int), minlength=18)
            assert {bool(cnt[a] * cnt[b] >= stage) for a, b in limbs} == {True, False}


def test_synthetic_inputs_hold_their_property():
    for s in PC.SYNTH_SETS:
        pk = PC.load_fixture(s, "coincident")["all_peaks"]
        a, b = pk[pk[:, 0] == 1][:, 1:3].tolist(), pk[pk[:, 0] == 2][:, 1:3].tolist()
        assert len([p for p in a if p in b]) == 1  # norm == 0 for exactly one neck / shoulder pair
        d = PC.load_fixture(s, "border")
        pk, mh, mw = d["all_peaks"], int(d["map_h"]), int(d["map_w"])
        assert np.any((pk[:, 1] == 0) | (pk[:, 2] == 0))
        assert np.any((pk[:, 1] == mw - 1) | (pk[:, 2] == mh - 1))
        assert len(d["conn"]) >= 3 and int(d["status"]) == 0


def test_peak_threshold_is_compared_in_f32():
    """heatmap_peak_thresh reaches the kernel as a float (post_shape), as the reference compares its
    f32 maps with it.  `peakf32`'s threshold is a double just below the f32 score of six_people's
    weakest peak and rounds UP to that score in f32: the reference drops the peak (not > itself),
    a compare in f64 would keep it -- and the rest of that joint's peaks stay."""
    t = PC.SETS["peakf32"]["heatmap_peak_thresh"]
    base, got = _default("six_people")["all_peaks"], PC.load_fixture("peakf32", "six_people")["all_peaks"]
    weakest = base[np.argmin(base[:, 3])]
    assert t < weakest[3] and float(np.float32(t)) == weakest[3]
    assert (base[:, 3] > t).sum() == len(base)            # f64 compare: every peak passes
    assert len(got) == len(base) - 1                       # the reference: all but that one
    assert not np.any((got[:, 1] == weakest[1]) & (got[:, 2] == weakest[2]) & (got[:, 0] == weakest[0]))
    # 0.15 (`thresh`) is no f32 value either, but no fixture pixel lies between it and its f32 neighbour
    assert float(np.float32(PC.SETS["thresh"]["heatmap_peak_thresh"])) != PC.SETS["thresh"]["heatmap_peak_thresh"]
