"""Generate the GPU-branch peak fixtures from the REFERENCE's own code.

Run in the build container only (it needs /root/reference, which does not exist on the GPU box), and
never imported by a test:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gpu_branch.py [set ...]

The reference's compute_peaks_from_heatmaps takes its ``else:`` branch (pose_detector.py:111-132) when
``cuda.get_array_module(heatmaps)`` is not NumPy.  That branch is pure array code apart from one
call, so it runs unchanged with these stand-ins:
  cuda.get_array_module  returns ``XP`` for a DeviceArray: an object that forwards every attribute to
                         NumPy (so ``xp == np`` is False) and hands its results back as DeviceArray, an
                         ndarray subclass with ``.get()``
  F.convolution_2d       returns an object whose ``.data`` is the zero-padded exact correlation with
                         the kernel it is GIVEN (the one the reference built): f64 sum over the f32
                         kernel, rounded once to f32 -- oracle.postproc.gpu_branch_filter's arithmetic.
                         cuDNN's accumulation order is unspecified; the exact sum is what every order
                         approximates
  self.gaussian_kernel   the reference's own create_gaussian_kernel(sigma, ksize)[None, None]
                         (pose_detector.py:34), set on an instance made with device = -1, whose
                         __init__ runs no device code
For every (set, case) of tests/gpu_branch_cases.py the reference's ``entity.params`` dict is updated
IN PLACE with the set's gaussian_sigma / ksize (and a case's heatmap_size), make_golden.py's
``run_reference`` runs the peaks above and the reference's unmodified compute_connections /
grouping_key_points / subsets_to_pose_array on them, and the defaults are put back.  Written to
tests/golden/gpu_branch/<set>__<case>.npz: the expected OUTPUTS only, the overrides as plain values
and the name of the input.  Two inputs are built here and kept in inputs__<case>.npz:
  subthresh  a 12 x 12 bump 0.0497 exp(-((y - 5)^2 + (x - 6)^2) / (2 5^2)) of joint 0 on a 96 x 96 map:
             every source value lies below heatmap_peak_thresh (1 - 1e-4), yet at sigma 0.5 the
             unnormalised kernel sums to 1.029 and the reference reports one peak
  seam       single-pixel bumps on 41 x 55 maps (a 320 x 432 map, 5 x 7 tiles of 64), their low-res
             columns / rows picked by search (seam_index) so that the upsampled bump's apex rounds to
             a pixel with x % 64 == 63, x % 64 == 0 (x > 0), and the same two for y; neck, right
             shoulder, right elbow and right hip on the four corners these span, joined by constant
             PAFs into one person, so the peaks also show in the poses

Asserted here, on the reference's output alone, for every fixture written:
  * decision margin (gpu_branch_cases.decision_margin on the filtered maps the reference itself
    thresholded) above 5e-6 of the map maximum.  Combinations replaced for falling short: twenty_720p
    (exact tie at (0.5, 3), 8.7e-7 at (2.5, 33)) by portrait_four; portrait_four at (0.7, 7) (3.5e-6)
    by neckless_merge (6.6e-5); one_person runs at the four sigma-2.5 sets with ksize <= 17 only
  * subthresh: max(source) < thresh (1 - 1e-4) and exactly one peak
  * border: a peak within 2 pixels of each of the four map edges
  * seam: the four seam conditions, on a map of at least 2 x 2 tiles, every seam peak part of a pose
  * oracle.postproc.compute_peaks_gpu_branch gives the identical array

The files are written with fixed zip timestamps, so a re-run reproduces them byte for byte.
"""
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import gpu_branch_cases as GC  # noqa: E402
from make_golden import install_stubs, run_reference  # noqa: E402
from make_golden_params import save_npz  # noqa: E402

OUT = GC.DIR


class DeviceArray(np.ndarray):
    """What the reference's GPU branch sees as a device array: NumPy semantics plus ``.get()``."""

    def get(self):
        return np.array(self, copy=True, subok=False)


def _device(v):
    if isinstance(v, np.ndarray):
        return v.view(DeviceArray)
    if isinstance(v, tuple):
        return tuple(_device(x) for x in v)
    return v


class _ArrayModule(object):
    """Module-like ``xp``: NumPy's functions, results as DeviceArray; not ``np`` itself."""

    def __getattr__(self, name):
        fn = getattr(np, name)
        if not callable(fn) or isinstance(fn, type):
            return fn
        return lambda *a, **k: _device(fn(*a, **k))


XP = _ArrayModule()
last_filtered = None  # the maps the reference thresholded in its last call (for the margin)


class _Variable(object):
    def __init__(self, data):
        self.data = data


def convolution_2d(x, W, b=None, stride=1, pad=0):
    """F.convolution_2d for the one call the reference makes (pose_detector.py:112): x (J, 1, H, W) f32,
    W (1, 1, k, k) f32, stride 1, pad k // 2 -> .data (J, 1, H, W) f32, the exact zero-padded
    correlation (f64 accumulation in the oracle's tap order) rounded once."""
    global last_filtered
    x, W = np.asarray(x), np.asarray(W)
    assert x.dtype == np.float32 and W.dtype == np.float32 and b is None and stride == 1
    assert x.ndim == 4 and x.shape[1] == 1 and W.shape[:2] == (1, 1) and W.shape[2] == W.shape[3]
    ks = W.shape[2]
    r = ks // 2
    assert ks % 2 == 1 and pad == r
    k = W[0, 0].astype(np.float64)
    J, _, H, Wd = x.shape
    p = np.zeros((J, H + 2 * r, Wd + 2 * r), np.float64)
    p[:, r:r + H, r:r + Wd] = x[:, 0]
    acc = np.zeros((J, H, Wd), np.float64)
    for dy in range(ks):
        for dx in range(ks):
            acc += k[dy, dx] * p[:, dy:dy + H, dx:dx + Wd]
    last_filtered = acc.astype(np.float32)
    return _Variable(last_filtered[:, None].view(DeviceArray))


class GpuBranchDetector(object):
    """The reference's PoseDetector with its heatmaps handed over as device arrays."""

    def __init__(self, pd):
        self._pd = pd

    def __getattr__(self, name):
        return getattr(self._pd, name)

    def compute_peaks_from_heatmaps(self, heatmaps):
        return self._pd.compute_peaks_from_heatmaps(np.asarray(heatmaps).view(DeviceArray))


def install_gpu_branch_stubs():
    install_stubs()
    ch = sys.modules["chainer"]
    ch.cuda.get_array_module = lambda *a: XP if isinstance(a[0], DeviceArray) else np
    ch.functions.convolution_2d = convolution_2d


# ---- the two inputs built here ----
def synth_subthresh():
    heat = np.zeros((19, 12, 12), np.float32)
    heat[18] = 1
    y, x = np.mgrid[0:12, 0:12].astype(np.float64)
    heat[0] = (0.0497 * np.exp(-((y - 5) ** 2 + (x - 6) ** 2) / (2 * 5.0 ** 2))).astype(np.float32)
    return np.zeros((38, 12, 12), np.float32), heat, 96, 96


SEAM_LOW = (41, 55)     # low-res rows, columns
SEAM_ORIG = (480, 640)  # -> a 320 x 432 map at heatmap_size 320
SEAM_MAP = (320, 432)


def seam_index(low, full, residue, taken=()):
    """The low-res index c, at least 3 from the ends and 6 from every index in ``taken``, whose
    align-corners position c (full - 1) / (low - 1) lies closest to a pixel p > 0 with p % 64 ==
    residue (and within 0.3 of it, so the apex rounds to p whatever the filter)."""
    best = None
    for c in range(3, low - 3):
        if any(abs(c - t) < 6 for t in taken):
            continue
        pos = c * (full - 1) / (low - 1)
        p = int(np.floor(pos + 0.5))
        if p > 0 and p % GC.KFT == residue and (best is None or abs(pos - p) < best[0]):
            best = (abs(pos - p), c, p)
    assert best is not None and best[0] < 0.3, (low, full, residue, best)
    return best[1], best[2]


def synth_seam():
    lh, lw = SEAM_LOW
    mh, mw = SEAM_MAP
    paf = np.zeros((38, lh, lw), np.float32)
    heat = np.zeros((19, lh, lw), np.float32)
    heat[18] = 1
    cx0, _ = seam_index(lw, mw, 0)
    cx63, _ = seam_index(lw, mw, GC.KFT - 1, (cx0,))
    cy0, _ = seam_index(lh, mh, 0)
    cy63, _ = seam_index(lh, mh, GC.KFT - 1, (cy0,))
    # one person of four joints on the corners of the rectangle the four indices span (a subset needs
    # n_subset_limbs_thresh = 3 joints to become a pose): neck -> right shoulder along x (limb 6 =
    # [1, 2], PAF channels 12, 13), shoulder -> right elbow along y (limb 7 = [2, 3], channels 14, 15),
    # neck -> right hip along y (limb 0 = [1, 8], channels 0, 1)
    heat[1, cy0, cx0] = 1.0
    heat[2, cy0, cx63] = 0.9
    heat[3, cy63, cx63] = 0.8
    heat[8, cy63, cx0] = 1.0
    paf[12, cy0 - 3:cy0 + 4, :] = np.sign(cx63 - cx0)
    paf[15, :, cx63 - 3:cx63 + 4] = np.sign(cy63 - cy0)
    paf[1, :, cx0 - 3:cx0 + 4] = np.sign(cy63 - cy0)
    return paf, heat, SEAM_ORIG[0], SEAM_ORIG[1]


OWN = {"subthresh": synth_subthresh, "seam": synth_seam}


def check_case(case, ref, heat_low, thresh):
    pk = ref["all_peaks"]
    mw, mh = ref["map_w"], ref["map_h"]
    if case == "subthresh":
        assert float(heat_low[:-1].max()) < float(np.float32(thresh)) * (1 - 1e-4), heat_low[:-1].max()
        assert len(pk) == 1, pk
    elif case == "border":
        x, y = pk[:, 1], pk[:, 2]
        assert np.any(x <= 2) and np.any(x >= mw - 3) and np.any(y <= 2) and np.any(y >= mh - 3), pk
    elif case == "seam":
        assert mw >= 2 * GC.KFT and mh >= 2 * GC.KFT
        for v in (pk[:, 1], pk[:, 2]):
            assert np.any(v % GC.KFT == GC.KFT - 1), pk
            assert np.any((v % GC.KFT == 0) & (v > 0)), pk
        on_seam = pk[np.isin(pk[:, 1] % GC.KFT, (0, GC.KFT - 1)) | np.isin(pk[:, 2] % GC.KFT, (0, GC.KFT - 1))]
        joints = ref["poses"].reshape(-1, 3)
        joints = joints[joints[:, 2] > 0][:, :2] / [ref["orig_w"] / mw, ref["orig_h"] / mh]
        for x, y in on_seam[:, 1:3]:
            assert np.any(np.all(np.abs(joints - [x, y]) < 1e-6, axis=1)), (x, y, joints)


_pd = None


def job(arg):
    set_name, case = arg
    from entity import params  # the reference's own dict (install_stubs put /root/reference first)
    from oracle import postproc
    ov = GC.overrides(set_name, case)
    paf_low, heat_low, orig_h, orig_w = OWN[case]() if case in OWN else GC.PC.load_inputs(case)
    before = dict(params)
    params.update(ov)
    try:
        _pd.gaussian_kernel = _pd.create_gaussian_kernel(params["gaussian_sigma"], params["ksize"])[None, None]
        ref = run_reference(GpuBranchDetector(_pd), paf_low, heat_low, orig_h, orig_w)
        thresh = params["heatmap_peak_thresh"]
    finally:
        params.update({k: before[k] for k in ov})
    assert params == before  # the defaults are back (a pool worker runs many jobs)
    assert last_filtered.shape == (18, ref["map_h"], ref["map_w"])
    margin = GC.decision_margin(last_filtered, thresh)
    assert margin > GC.MARGIN_FLOOR, (set_name, case, margin)
    check_case(case, ref, heat_low, thresh)
    restated = postproc.compute_peaks_gpu_branch(postproc.resize_images(heat_low, ref["map_h"], ref["map_w"]),
                                                 dict(postproc.PARAMS, **ov))
    assert np.array_equal(restated.reshape(-1, 5), ref["all_peaks"]), (set_name, case)
    out = {k: ref[k] for k in GC.OUTPUT_KEYS if k in ref}
    for k, v in ov.items():
        out["override__" + k] = np.asarray(v)
    out["input"] = np.asarray(case)
    save_npz(GC.fixture_path(set_name, case), out)
    return "%-8s %-14s peaks=%4d conns=%4d persons=%s status=%d margin=%.3g" % (
        set_name, case, len(ref["all_peaks"]), len(ref.get("conn", [])),
        ref["poses_shape"][0] if "poses_shape" in ref else "-", ref["status"], margin)


def main(argv):
    global _pd
    install_gpu_branch_stubs()
    import pose_detector  # the reference, from /root/reference
    from entity import params
    _pd = pose_detector.PoseDetector(model=object())  # device = -1: no device code runs
    for p in GC.pairs():
        assert set(GC.overrides(*p)) <= set(params), p
    # one oracle call before the pool forks: the C oracle builds itself on first use, and the
    # workers must not all build it at once
    from oracle import postproc
    postproc.resize_images(np.zeros((1, 2, 2), np.float32), 4, 4)
    os.makedirs(OUT, exist_ok=True)
    for case, make in OWN.items():
        paf_low, heat_low, oh, ow = make()
        save_npz(os.path.join(OUT, "inputs__%s.npz" % case),
                 {"paf_low": paf_low, "heat_low": heat_low, "orig_h": oh, "orig_w": ow})
    jobs = [p for p in GC.pairs() if not argv or p[0] in argv]
    jobs.sort(key=lambda p: -GC.SETS[p[0]][1])  # the largest kernels first
    with multiprocessing.get_context("fork").Pool(min(8, os.cpu_count() or 1)) as pool:
        for line in pool.imap(job, jobs):
            print(line, flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
