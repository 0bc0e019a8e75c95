"""The (gaussian_sigma, ksize) sets and cases of the GPU-branch peak fixtures (tests/golden/gpu_branch/,
made by tests/golden/make_golden_gpu_branch.py from the reference's own ``else:`` branch of
compute_peaks_from_heatmaps under a NumPy-backed ``xp``) and the helpers that read them.

A fixture ``<set>__<case>.npz`` holds the reference's OUTPUTS for the inputs of a golden
(tests/golden/<case>.npz), of a synthetic input of the parameter fixtures
(tests/golden/params/inputs__<case>.npz) or of one built for this directory
(tests/golden/gpu_branch/inputs__<case>.npz), with ``entity.params`` updated by the overrides the
fixture records."""
import os

import numpy as np

import params_cases as PC

DIR = os.path.join(PC.GOLDEN, "gpu_branch")
KFT = 64  # heat_fused's output tile edge (postproc.hip kFT), asserted against the source by the tests

# set -> (gaussian_sigma, ksize).  Radius 8 is the compile-time instantiation heat_fused<HeatLow, 8, true>;
# every other radius runs <HeatLow, 0, true>: 1 (the smallest), 2, 3, 4 and 16 (kMaxR).
SETS = {
    "s25_k3": (2.5, 3),
    "s25_k5": (2.5, 5),
    "s25_k9": (2.5, 9),
    "s25_k17": (2.5, 17),
    "s25_k33": (2.5, 33),
    "s10_k9": (1.0, 9),
    "s07_k7": (0.7, 7),
    # the unnormalised kernel sums to MORE than 1 here (test_tap_sum_table): the tile early-out
    "s05_k3": (0.5, 3),
    "s05_k5": (0.5, 5),
}
EVERY_SET = list(SETS)
# case -> the sets it runs at.  twenty_720p is left out on purpose: its reference peaks hold an exact
# tie at (0.5, 3) (decision margin 0) and a margin of 8.7e-7 at (2.5, 33); noise_crowd stays with the
# ksize-17 test of test_gpu_peak_mode.py.
CASES = {
    "six_people": EVERY_SET,
    # (0.7, 7) leaves portrait_four a margin of 3.5e-6, below MARGIN_FLOOR: neckless_merge stands in there
    "portrait_four": [s for s in EVERY_SET if s != "s07_k7"],
    "neckless_merge": ["s07_k7"],
    "one_person": ["s25_k3", "s25_k5", "s25_k9", "s25_k17"],
    # tests/golden/params/inputs__*.npz: peaks in the outermost rows / columns (zero padding, not the
    # CPU branch's reflection), two joints' peaks on one pixel
    "border": EVERY_SET,
    "coincident": EVERY_SET,
    # a 12 x 12 bump whose maximum stays BELOW heatmap_peak_thresh * (1 - 1e-4), on a 96 x 96 map: the
    # kernel's sum above 1 lifts exactly one filtered value over the threshold
    "subthresh": ["s05_k5", "s05_k3"],
    # single-pixel bumps whose peaks fall in the last column / row of a tile and in the first of the next
    "seam": ["s25_k5", "s25_k33", "s05_k5"],
}
# overrides of entity.params a case adds to its set's gaussian_sigma / ksize
CASE_OVERRIDES = {"subthresh": {"heatmap_size": 96}}
OWN_INPUTS = ["subthresh", "seam"]  # built by the generator, kept in DIR
MARGIN_FLOOR = 5e-6  # every fixture's decision margin (decision_margin below) lies above this

OUTPUT_KEYS = PC.OUTPUT_KEYS


def overrides(set_name, case):
    sigma, ksize = SETS[set_name]
    return dict({"gaussian_sigma": sigma, "ksize": ksize}, **CASE_OVERRIDES.get(case, {}))


def pairs():
    """Every (set, case) that has a fixture, in generation order."""
    return [(s, c) for c, sets in CASES.items() for s in sets]


def fixture_path(set_name, case):
    return os.path.join(DIR, "%s__%s.npz" % (set_name, case))


def load_fixture(set_name, case):
    return dict(np.load(fixture_path(set_name, case)))


def load_inputs(case):
    """paf_low, heat_low, orig_h, orig_w of a case."""
    if case not in OWN_INPUTS:
        return PC.load_inputs(case)
    d = np.load(os.path.join(DIR, "inputs__%s.npz" % case))
    return d["paf_low"], d["heat_low"], int(d["orig_h"]), int(d["orig_w"])


def tap_sum_2d(sigma, ksize):
    """(sum of g)^2 of the 1-D factor g(d) = exp(-d^2 / 2 s^2) / sqrt(2 pi s^2), d = -r .. r
    (host_pack.hpp gpu_branch_taps): the sum of the reference's unnormalised ksize x ksize kernel."""
    r = ksize // 2
    d = np.arange(-r, r + 1, dtype=np.float64)
    return float((np.exp(-0.5 * d * d / (sigma * sigma)) / np.sqrt(2.0 * np.pi * sigma * sigma)).sum()) ** 2


def decision_margin(filtered, thresh):
    """Relative room a rounding difference has before one peak decision of the GPU branch flips, on
    its filtered (J, H, W) maps: for a peak, its smallest gap to the threshold or a neighbour; for any
    other pixel, its largest failing gap (all of them must flip to make it a peak).  Neighbours
    outside the map count as 0; relative to the map maximum."""
    f = np.asarray(filtered).astype(np.float64)
    pad = np.pad(f, ((0, 0), (1, 1), (1, 1)))
    g = [f - np.float64(np.float32(thresh))]
    for dy, dx in ((0, 1), (2, 1), (1, 0), (1, 2)):
        g.append(f - pad[:, dy:dy + f.shape[1], dx:dx + f.shape[2]])
    g = np.stack(g)
    peak = (g[0] > 0) & np.all(g[1:] >= 0, axis=0)
    m_peak = np.where(peak, np.abs(g).min(axis=0), np.inf)
    fail = np.where(np.concatenate([(g[0] <= 0)[None], g[1:] < 0]), np.abs(g), 0.0)
    m_non = np.where(~peak, fail.max(axis=0), np.inf)
    return min(float(m_peak.min()), float(m_non.min())) / max(float(f.max()), 1e-30)


def separable_like_the_device(h, sigma=2.5, ksize=17):
    """The device's arithmetic for the GPU branch (postproc.hip heat_fused<.., G>): the 1-D factor
    g(d) = exp(-d^2 / 2 s^2) / sqrt(2 pi s^2) (host_pack.hpp gpu_branch_taps), a vertical then a
    horizontal pass in f64 over zero-padded f32 maps, rounded to f32 after each pass."""
    r = ksize // 2
    d = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-0.5 * d * d / (sigma * sigma)) / np.sqrt(2.0 * np.pi * sigma * sigma)
    J, H, W = h.shape
    p = np.zeros((J, H + 2 * r, W), np.float64)
    p[:, r:r + H] = h
    v = sum(g[k] * p[:, k:k + H] for k in range(ksize)).astype(np.float32)
    q = np.zeros((J, H, W + 2 * r), np.float64)
    q[:, :, r:r + W] = v
    return sum(g[k] * q[:, :, k:k + W] for k in range(ksize)).astype(np.float32)
