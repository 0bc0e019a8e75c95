"""The non-default parameter sets of the post-process fixtures (tests/golden/params/, made by
tests/golden/make_golden_params.py from the reference's own code) and the helpers that read them.

A fixture ``<set>__<case>.npz`` holds the reference's OUTPUTS for the inputs of the golden ``<case>``
(tests/golden/<case>.npz) under ``entity.params`` updated with the set's overrides; the two synthetic
cases keep their inputs in ``inputs__<case>.npz`` next to the fixtures."""
import glob
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
PARAMS_DIR = os.path.join(GOLDEN, "params")
CSRC = os.path.join(os.path.dirname(HERE), "chainer_realtime_multi-person_pose_estimation_amd", "csrc")

# set -> overrides of entity.params, and what the set reaches in the kernels
SETS = {
    # limb_pairs_body's restatement of NumPy's pairwise sum: loop body without a tail (the kernel's
    # maximum), 8 accumulators + a tail of 5, the sequential form, the minimum (endpoints only)
    "integ16": {"n_integ_points": 16, "n_integ_points_thresh": 12},
    "integ13": {"n_integ_points": 13, "n_integ_points_thresh": 9},
    "integ7": {"n_integ_points": 7, "n_integ_points_thresh": 5},
    "integ2": {"n_integ_points": 2, "n_integ_points_thresh": 1},
    # the length penalty active for most pairs (zero for most at the defaults)
    "length": {"limb_length_ratio": 0.25, "length_penalty_value": 0.9},
    "thresh": {"heatmap_peak_thresh": 0.15, "inner_product_thresh": 0.2, "n_subset_limbs_thresh": 6,
               "subset_score_thresh": 0.45},
    # `thresh`'s 0.45 drops no subset of these inputs (their score / joint-count ratios start at 1.27):
    # 1.45 drops one of six_people's, two of twenty_720p's and three of neckless_merge's
    "score": {"subset_score_thresh": 1.45},
    # a double one ulp (of f64) below the f32 score 0.7480858564376831 of six_people's weakest peak (joint
    # 5 at (273, 66)): the reference compares `heatmap > thresh` in f32, where the threshold rounds UP to
    # that score and the peak is dropped; a compare in f64 would keep it
    "peakf32": {"heatmap_peak_thresh": 0.748085856437683},
    # 4x upsample, 3x3 and 3x6 tiles; downsample, one tile, the unstaged low-res window
    "map184": {"heatmap_size": 184},
    "map40": {"heatmap_size": 40},
    # run-time Gaussian radius 4 together with a non-default map
    "sigma1_map248": {"gaussian_sigma": 1.0, "heatmap_size": 248},
}
GOLDEN_CASES = ["one_person", "six_people", "noise_crowd", "portrait_four", "twenty_720p", "neckless_merge"]
# the reference takes 45-115 s per set on noise_crowd at full density: only where it adds a branch
NOISE_SETS = ["integ2", "integ16", "thresh", "map184"]
# synthetic inputs (make_golden_params.py), each at the defaults and at both ends of n_integ_points
SYNTH_CASES = ["coincident", "border"]
SYNTH_SETS = ["default", "integ2", "integ16"]
# noise_crowd's network maps tiled 2 x 2 (92 x 92, as a 736-pixel network input gives): a limb's two
# low-res PAF planes no longer fit limb_pairs_low's LDS next to the tap tables (`tables` 1).  Only
# with `thresh`, which leaves the reference few enough peaks to finish in minutes.
TILED_CASES = {"noise_crowd_2x2": ("noise_crowd", 2, 2)}
TILED_SETS = ["thresh"]
ALL_SETS = dict(SETS, default={})

# which stage of the reference a set's parameters feed first
STAGE_PEAKS = ["thresh", "peakf32", "map184", "map40", "sigma1_map248"]
STAGE_CONNECTIONS = ["integ16", "integ13", "integ7", "integ2", "length"]
STAGE_PERSONS = ["thresh", "score"]

OUTPUT_KEYS = ["all_peaks", "conn", "conn_off", "subsets", "poses", "poses_shape", "scores", "status", "map_h",
               "map_w"]


def pairs():
    """Every (set, case) that has a fixture, in generation order."""
    out = []
    for s in SETS:
        for c in GOLDEN_CASES:
            if c != "noise_crowd" or s in NOISE_SETS:
                out.append((s, c))
    for s in SYNTH_SETS:
        for c in SYNTH_CASES:
            out.append((s, c))
    for s in TILED_SETS:
        for c in TILED_CASES:
            out.append((s, c))
    return out


def fixture_path(set_name, case):
    return os.path.join(PARAMS_DIR, "%s__%s.npz" % (set_name, case))


def load_fixture(set_name, case):
    return dict(np.load(fixture_path(set_name, case)))


def load_inputs(case):
    """paf_low, heat_low, orig_h, orig_w of a case: an existing golden's (tiled for a TILED case:
    same frame size, so the post-process map stays as it is), or a synthetic case's own."""
    if case in TILED_CASES:
        base, ny, nx = TILED_CASES[case]
        paf_low, heat_low, oh, ow = load_inputs(base)
        return np.tile(paf_low, (1, ny, nx)), np.tile(heat_low, (1, ny, nx)), oh, ow
    path = os.path.join(PARAMS_DIR, "inputs__%s.npz" % case) if case in SYNTH_CASES else \
        os.path.join(GOLDEN, case + ".npz")
    d = np.load(path)
    return d["paf_low"], d["heat_low"], int(d["orig_h"]), int(d["orig_w"])


def overrides_of(fixture):
    """The overrides a fixture records (``override__<name>`` entries) as plain Python values."""
    return {k[len("override__"):]: v.item() for k, v in fixture.items() if k.startswith("override__")}


def fixture_files():
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(PARAMS_DIR, "*.npz")))


def kernel_constant(name, source="postproc.hip"):
    """``constexpr int[64_t] <name> = <integer>;`` as the kernel source has it."""
    with open(os.path.join(CSRC, source)) as f:
        m = re.search(r"constexpr\s+int(?:64_t)?\s+%s\s*=\s*(\d+)\s*;" % re.escape(name), f.read())
    assert m, "constant %s not found in %s" % (name, source)
    return int(m.group(1))
