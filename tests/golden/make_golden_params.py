"""Generate the non-default-parameter post-process fixtures from the REFERENCE's own code.

Run in the build container only (it needs /root/reference, which does not exist on the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_params.py [set ...]

For every parameter set of tests/params_cases.py the reference's ``entity.params`` dict is updated IN
PLACE (pose_detector.py reads that module-level dict), make_golden.py's ``run_reference`` runs the
reference's unmodified compute_peaks_from_heatmaps / compute_connections / grouping_key_points /
subsets_to_pose_array on the network maps of an existing golden (tests/golden/<case>.npz: paf_low,
heat_low, orig_h, orig_w), and the defaults are put back.  Written to
tests/golden/params/<set>__<case>.npz: the expected OUTPUTS only, the overrides as plain values and
the name of the input golden.  The inputs are read from the goldens, not copied (one case tiles a
golden's maps 2 x 2 on the fly: params_cases.TILED_CASES).

Two synthetic inputs are built here (a few pixels set on 46 x 46 maps, like make_golden.py's
no_person) and kept in tests/golden/params/inputs__<case>.npz:
  coincident  a neck and a right shoulder (limb [1, 2]) peak at the SAME map pixel, next to a normal
              pair: the ``norm == 0: continue`` of compute_candidate_connections (pose_detector.py:141)
  border      peaks in the map's outermost rows and columns joined by constant PAFs: the line
              integral's endpoints sit on the edge, the Gaussian's reflected boundary carries a peak

The files are written with fixed zip timestamps, so a re-run reproduces them byte for byte.
"""
import io
import multiprocessing
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import params_cases as PC  # noqa: E402
from make_golden import LegacyIndexArray, install_stubs, run_reference  # noqa: E402,F401

OUT = PC.PARAMS_DIR


def save_npz(path, arrays):
    """np.savez_compressed with sorted members and a fixed timestamp (byte-identical re-runs)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, buf.getvalue())


def blank_maps():
    heat = np.zeros((19, 46, 46), np.float32)
    heat[18] = 1
    return np.zeros((38, 46, 46), np.float32), heat


def synth_coincident():
    """Neck (1) and right shoulder (2) bumps on the same low-res pixel -> one map coordinate for
    both peaks; a second, ordinary neck / shoulder pair; limb 6 = [1, 2] has PAF channels 12, 13."""
    paf, heat = blank_maps()
    heat[1, 20, 20] = 1.0
    heat[2, 20, 20] = 1.0
    heat[1, 24, 28] = 1.0
    heat[2, 26, 36] = 0.9
    paf[12, 14:32, :] = 1.0   # x component: every pair of this band points along +x
    paf[13, 14:32, :] = 0.25
    return paf, heat


def synth_border():
    """Bumps in low-res row 0, the last row, column 0 and the last column (align-corners upsampling
    maps them to the map's outermost rows / columns), joined by constant PAFs along each limb."""
    paf, heat = blank_maps()
    heat[1, 0, 10] = 1.0     # neck, top row
    heat[8, 45, 10] = 1.0    # right hip, bottom row: limb 0 = [1, 8], PAF channels 0, 1
    paf[1, :, 6:15] = 1.0    # y component down column 10
    heat[1, 20, 0] = 0.9     # a second neck, left column
    heat[2, 20, 45] = 1.0    # right shoulder, right column: limb 6 = [1, 2], channels 12, 13
    paf[12, 16:25, :] = 1.0  # x component along row 20
    heat[3, 45, 45] = 1.0    # right elbow in the corner: limb 7 = [2, 3], channels 14, 15
    paf[15, :, 41:46] = 1.0  # y component down the last columns
    return paf, heat


SYNTH = {"coincident": synth_coincident, "border": synth_border}
SYNTH_ORIG = (480, 480)


def check_synthetic(case, ref):
    """The property each synthetic input exists for, on the reference's own peaks."""
    pk = ref["all_peaks"]
    if case == "coincident":
        a, b = pk[pk[:, 0] == 1], pk[pk[:, 0] == 2]
        same = [(x, y) for x, y in a[:, 1:3].tolist() if [x, y] in b[:, 1:3].tolist()]
        assert len(a) == 2 and len(b) == 2 and len(same) == 1, (a, b)
    else:
        mw, mh = ref["map_w"], ref["map_h"]
        assert np.any((pk[:, 1] == 0) | (pk[:, 2] == 0)), pk
        assert np.any((pk[:, 1] == mw - 1) | (pk[:, 2] == mh - 1)), pk
        assert len(ref["conn"]) >= 3, ref["conn"]


_pd = None


def job(arg):
    set_name, case = arg
    from entity import params  # the reference's own dict (install_stubs put /root/reference first)
    ov = PC.ALL_SETS[set_name]
    if case in SYNTH:
        paf_low, heat_low = SYNTH[case]()
        orig_h, orig_w = SYNTH_ORIG
    else:
        paf_low, heat_low, orig_h, orig_w = PC.load_inputs(case)
    before = dict(params)
    params.update(ov)
    try:
        ref = run_reference(_pd, paf_low, heat_low, orig_h, orig_w)
    finally:
        params.update({k: before[k] for k in ov})
    assert params == before  # the defaults are back (a pool worker runs many jobs)
    if case in SYNTH:
        check_synthetic(case, ref)
    out = {k: ref[k] for k in PC.OUTPUT_KEYS if k in ref}
    for k, v in ov.items():
        out["override__" + k] = np.asarray(v)
    out["input"] = np.asarray(case)
    save_npz(PC.fixture_path(set_name, case), out)
    return "%-14s %-16s peaks=%4d conns=%4d persons=%s status=%d" % (
        set_name, case, len(ref["all_peaks"]), len(ref.get("conn", [])),
        ref["poses_shape"][0] if "poses_shape" in ref else "-", ref["status"])


def main(argv):
    global _pd
    install_stubs()
    import pose_detector  # the reference, from /root/reference
    from entity import params
    _pd = pose_detector.PoseDetector(model=object())
    for ov in PC.SETS.values():
        assert set(ov) <= set(params), ov
    # one oracle call before the pool forks: the C oracle builds itself on first use, and the
    # workers must not all build it at once
    from oracle import postproc
    postproc.resize_images(np.zeros((1, 2, 2), np.float32), 4, 4)
    os.makedirs(OUT, exist_ok=True)
    for case, make in SYNTH.items():
        paf_low, heat_low = make()
        save_npz(os.path.join(OUT, "inputs__%s.npz" % case),
                 {"paf_low": paf_low, "heat_low": heat_low, "orig_h": SYNTH_ORIG[0], "orig_w": SYNTH_ORIG[1]})
    jobs = [p for p in PC.pairs() if not argv or p[0] in argv]
    jobs.sort(key=lambda p: not p[1].startswith("noise_crowd"))  # the slow ones first
    with multiprocessing.get_context("fork").Pool(min(8, os.cpu_count() or 1)) as pool:
        for line in pool.imap(job, jobs):
            print(line, flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
