"""COCO keypoint matching on the GPU (op_keypoint_match / op_keypoint_match_staged,
csrc/keypoint.hip) held bit for bit to ``keypoint_eval.match_np`` on every output, the staged entry
held to the host entry on the fetched rows, ``evaluate`` to ``evaluate_np``, and the refusals."""
import ctypes

import numpy as np
import pytest

import keypoint_cases as cases
from conftest import load_golden, pkg_module

pytestmark = pytest.mark.gpu

H = W = 480  # the network input is 368 x 368: the 46 x 46 maps of six_people fit
FRAMES = np.random.default_rng(32).integers(0, 256, (3, H, W, 3), dtype=np.uint8)
KEYS = ("dt_order", "dt_scores", "oks", "dt_match", "dt_ignore", "gt_match", "gt_ignore")


@pytest.fixture(scope="module")
def K():
    return pkg_module("keypoint_eval")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(got, want, where):
    for key in KEYS:
        g, w = got[key], want[key]
        assert g.dtype == w.dtype and g.shape == w.shape, (where, key, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(_bits(g), _bits(w)), (where, key)


def _blob(records):
    return b"".join(np.ascontiguousarray(r[k]).tobytes() for r in records for k in KEYS)


def test_kernel_equals_match_np_on_every_output(lib, K):
    frames, refs = cases.all_frames(), cases.references(K)
    assert len(frames) >= 48
    dets, gts = [f[1] for f in frames], [f[2] for f in frames]
    got = lib.keypoint_match(dets, gts, max_dets=cases.MAX_DETS)
    print("%d frames, %d detections, %d ground truths, uploads + kernel %.3f ms" % (
        len(frames), sum(len(d[1]) for d in dets), sum(len(g[1]) for g in gts), lib.keypoint_last_ms(0)))
    bad = []
    for (name, _, _), g, w in zip(frames, got, refs):
        for key in KEYS:
            if g[key].dtype != w[key].dtype or g[key].shape != w[key].shape or not np.array_equal(_bits(g[key]), _bits(w[key])):
                bad.append((name, key))
    assert not bad, bad
    # one call per frame gives the same bytes as the frame's part of the one call
    names = [f[0] for f in frames]
    for name in ("128_ground_truths_the_cap", "nan_score", "scene_40"):
        i = names.index(name)
        alone = lib.keypoint_match([dets[i]], [gts[i]], max_dets=cases.MAX_DETS)
        assert _blob(alone) == _blob([got[i]]), name
    # the OKS matrix is optional; the other outputs do not change without it
    lean = lib.keypoint_match(dets, gts, max_dets=cases.MAX_DETS, want_oks=False)
    assert all("oks" not in r for r in lean)
    for g, r in zip(got, lean):
        assert all(np.array_equal(_bits(g[k]), _bits(r[k])) for k in KEYS if k != "oks")
    assert lib.keypoint_match([], []) == []


def test_other_constants(lib, K):
    """max_dets 1 and 64, one threshold, four area ranges, other sigmas: the arguments are read."""
    frames = cases.all_frames()
    pick = [f for f in frames if f[0] in ("25_detections_cut_to_20", "70_ground_truths", "scene_41", "neither")]
    for max_dets, thrs, rng, sig in ((1, [0.5], [[0, 1e10]], K.KPT_SIGMAS),
                                     (64, np.linspace(0.05, 0.8, 16), [[0, 1e10], [0, 2000], [2000, 5000], [5000, 1e10]],
                                      K.KPT_SIGMAS[::-1] * 1.5)):
        got = lib.keypoint_match([f[1] for f in pick], [f[2] for f in pick], max_dets=max_dets, thrs=thrs, area_rng=rng,
                                 sigmas=sig)
        for (name, d, g), rec in zip(pick, got):
            _same(rec, K.match_np(d[0], d[1], *g, max_dets=max_dets, thrs=thrs, area_rng=rng, sigmas=sig), name)


def test_evaluate_equals_evaluate_np(lib, K):
    frames = cases.all_frames()
    dets, gts = [f[1] for f in frames], [f[2] for f in frames]
    want = K.evaluate_np(dets, gts)
    got = K.evaluate(dets, gts)
    print(K.format_summary(got["stats"])[0])
    assert np.array_equal(_bits(got["stats"]), _bits(want["stats"]))
    assert np.array_equal(got["precision"], want["precision"]) and np.array_equal(got["recall"], want["recall"])
    assert 0 < got["stats"][0] < 1 and (got["stats"] > -1).all()


# ---- the staged entry ----

@pytest.fixture(scope="module")
def pd(rand_weights):
    """A PoseDetector whose staged step post-processes staged maps: the six_people maps for frames
    0 and 2 and all-zero maps for frame 1 (7 persons, none, 7 persons)."""
    det = pkg_module("pose_detector").PoseDetector("posenet", model=rand_weights, max_batch=3)
    d = load_golden("six_people")
    maps = np.zeros((3, 57, 46, 46), np.float32)
    maps[0] = maps[2] = np.concatenate([d["paf_low"], d["heat_low"]])
    ctx = det.staged_context()
    ctx.stage_frames(FRAMES)
    ctx.stage_maps(maps)
    ctx.use_staged_maps(True)
    ctx.run_staged()
    ctx.synchronize()
    yield det
    ctx.use_staged_maps(False)


@pytest.fixture(scope="module")
def staged(pd, K):
    """The fetched rows, and ground truths made from them: perturbed by a seeded few pixels, some
    joints hidden, one person dropped, one marked crowd."""
    ctx = pd.staged_context()
    results = ctx.fetch_results(0, 3)
    assert [len(r[0]) for r in results] == [7, 0, 7]
    rng = np.random.default_rng(33)
    gts = []
    for i, (poses, _, _) in enumerate(results):
        kp = K.to_coco(poses)
        if i == 0:
            kp = kp[:-1]  # one person has no ground truth
        found = kp[:, :, 2] > 0
        kp[:, :, :2] += rng.normal(0.0, 3.0, kp[:, :, :2].shape)
        kp[:, :, 2] = np.where(found & (rng.uniform(size=found.shape) < 0.8), 2.0, 0.0)
        kp[kp[:, :, 2] == 0] = 0.0
        area, bbox = np.zeros(len(kp)), np.zeros((len(kp), 4))
        for g, k in enumerate(kp):
            v = k[k[:, 2] > 0]
            x0, y0, x1, y1 = v[:, 0].min(), v[:, 1].min(), v[:, 0].max(), v[:, 1].max()
            bbox[g] = [x0, y0, x1 - x0, y1 - y0]
            area[g] = 0.6 * (x1 - x0) * (y1 - y0)
        crowd = np.zeros(len(kp), np.uint8)
        if i == 2:
            crowd[3] = 1
        gts.append((kp, area, bbox, crowd.copy(), crowd))
    return {"ctx": ctx, "results": results, "gts": gts}


def test_staged_equals_the_host_entry(lib, K, pd, staged):
    ctx, results, gts = staged["ctx"], staged["results"], staged["gts"]
    raw_before = [(p.tobytes(), s.tobytes()) for p, s, _ in ctx.fetch_results(0, 3)]
    dets = [(K.to_coco(p), s) for p, s, _ in results]
    for max_dets in (20, 4):  # 4: fewer than the persons found
        host = lib.keypoint_match(dets, gts, max_dets=max_dets)
        status, got = ctx.keypoint_match(0, 3, gts, max_dets=max_dets, want_oks=True)
        print("staged, max_dets %d: uploads + kernel %.3f ms" % (max_dets, lib.keypoint_last_ms(0)))
        assert list(status) == [lib.OP_OK] * 3
        for i in range(3):
            _same(got[i], host[i], "frame %d, max_dets %d" % (i, max_dets))
            _same(got[i], K.match_np(dets[i][0], dets[i][1], *gts[i], max_dets=max_dets), "statement, frame %d" % i)
        assert [len(r["dt_order"]) for r in got] == [min(7, max_dets), 0, min(7, max_dets)]
    assert (got[0]["dt_match"] >= 0).any() and (host[2]["dt_ignore"] != 0).any()
    # a sub-range, and the records of evaluate_staged
    _, one = ctx.keypoint_match(2, 1, gts[2:], want_oks=True)
    _same(one[0], lib.keypoint_match(dets[2:], gts[2:])[0], "frame 2 alone")
    recs = K.evaluate_staged(pd, 0, 3, gts)
    want = lib.keypoint_match(dets, gts, want_oks=False)
    for r, w in zip(recs, want):
        assert "oks" not in r and all(np.array_equal(_bits(r[k]), _bits(w[k])) for k in KEYS if k != "oks")
    stats = K.summarize(K.accumulate_np(recs))
    assert np.array_equal(_bits(stats), _bits(K.evaluate_np(dets, gts)["stats"])) and stats[0] > 0
    # the result rows were only read
    raw_after = [(p.tobytes(), s.tobytes()) for p, s, _ in ctx.fetch_results(0, 3)]
    assert raw_after == raw_before


# ---- refusals ----

class _Call(object):
    """The arguments of one op_keypoint_match call on two small frames, each replaceable; outputs
    pre-filled so that a write would show."""

    def __init__(self, lib, K):
        frames = [f for f in cases.all_frames() if f[0] in ("scene_42", "scene_43")]
        dets, gts = [f[1] for f in frames], [f[2] for f in frames]
        self.lib = lib
        self.n = 2
        self.a = {
            "dt_off": np.array([0, len(dets[0][1]), len(dets[0][1]) + len(dets[1][1])], np.int32),
            "dt_kpts": np.ascontiguousarray(np.concatenate([d[0] for d in dets])),
            "dt_scores": np.ascontiguousarray(np.concatenate([d[1] for d in dets])),
            "gt_off": np.array([0, len(gts[0][1]), len(gts[0][1]) + len(gts[1][1])], np.int32),
            "gt_kpts": np.ascontiguousarray(np.concatenate([g[0] for g in gts])),
            "gt_area": np.ascontiguousarray(np.concatenate([g[1] for g in gts])),
            "gt_bbox": np.ascontiguousarray(np.concatenate([g[2] for g in gts])),
            "gt_ignore": np.ascontiguousarray(np.concatenate([g[3] for g in gts]), np.uint8),
            "gt_crowd": np.ascontiguousarray(np.concatenate([g[4] for g in gts]), np.uint8),
            "max_dets": 20, "n_thrs": 10, "thrs": K.OKS_THRS.copy(), "n_areas": 3,
            "rng": np.array(K.AREA_RNG, np.float64), "sig": K.KPT_SIGMAS.copy(),
        }
        G = int(self.a["gt_off"][-1])
        self.out = {"dt_order": np.full((2, 20), 77, np.int32), "oks": np.full(20 * G, 77.0),
                    "dt_match": np.full((2, 3, 10, 20), 77, np.int32), "dt_ignore": np.full((2, 3, 10, 20), 77, np.uint8),
                    "gt_match": np.full(30 * G, 77, np.int32), "gt_ig": np.full(3 * G, 77, np.uint8)}
        self.joint_map = K.joint_map()
        self.extra = {"status": np.full(2, 77, np.int32), "count": np.full(2, 77, np.int32), "scores": np.full((2, 20), 77.0)}

    def _args(self, a, out):
        p = self.lib.ptr
        return [p(a["gt_off"]), p(a["gt_kpts"]), p(a["gt_area"]), p(a["gt_bbox"]), p(a["gt_ignore"]), p(a["gt_crowd"]),
                a["max_dets"], a["n_thrs"], p(a["thrs"]), a["n_areas"], p(a["rng"]), p(a["sig"])], [
                    p(out["dt_order"]), p(out["oks"]), p(out["dt_match"]), p(out["dt_ignore"]), p(out["gt_match"]), p(out["gt_ig"])]

    def host(self, n=None, **repl):
        a, out = dict(self.a), dict(self.out)
        for k, v in repl.items():
            (out if k in out else a)[k] = v
        p = self.lib.ptr
        mid, outs = self._args(a, out)
        return self.lib.lib().op_keypoint_match(0, self.n if n is None else n, p(a["dt_off"]), p(a["dt_kpts"]),
                                                p(a["dt_scores"]), *(mid + outs))

    def staged(self, ctx, first, n, **repl):
        a, out, extra = dict(self.a), dict(self.out), dict(self.extra)
        jm = repl.pop("joint_map", self.joint_map)
        for k, v in repl.items():
            (out if k in out else extra if k in extra else a)[k] = v
        p = self.lib.ptr
        mid, outs = self._args(a, out)
        return self.lib.lib().op_keypoint_match_staged(ctx.h if ctx is not None else None, first, n, p(jm), *(
            mid + [p(extra["status"]), p(extra["count"]), p(extra["scores"])] + outs))

    def untouched(self):
        return all((v == 77).all() for v in list(self.out.values()) + list(self.extra.values()))


def _with(arr, index, value):
    arr = arr.copy()
    arr[index] = value
    return arr


def test_refusals_of_the_host_entry(lib, K):
    c = _Call(lib, K)
    a = c.a
    bad = [
        ("null dt_offsets", dict(dt_off=None)), ("null dt_kpts", dict(dt_kpts=None)), ("null dt_scores", dict(dt_scores=None)),
        ("null gt_offsets", dict(gt_off=None)), ("null gt table", dict(gt_kpts=None)), ("null gt table", dict(gt_area=None)),
        ("null gt table", dict(gt_bbox=None)), ("null gt table", dict(gt_ignore=None)), ("null gt table", dict(gt_crowd=None)),
        ("null thrs", dict(thrs=None)), ("null area_rng", dict(rng=None)), ("null sigmas", dict(sig=None)),
        ("null output", dict(dt_order=None)), ("null output", dict(dt_match=None)), ("null output", dict(dt_ignore=None)),
        ("null output", dict(gt_match=None)), ("null output", dict(gt_ig=None)),
        ("dt offsets decrease", dict(dt_off=np.array([0, a["dt_off"][2], a["dt_off"][1]], np.int32))),
        ("dt offsets start", dict(dt_off=_with(a["dt_off"], 0, 1))),
        ("gt offsets decrease", dict(gt_off=np.array([0, a["gt_off"][2], a["gt_off"][1]], np.int32))),
        ("gt offsets start", dict(gt_off=_with(a["gt_off"], 0, 1))),
        ("max_dets 0", dict(max_dets=0)), ("max_dets 65", dict(max_dets=65)),
        ("n_thrs 0", dict(n_thrs=0)), ("n_thrs 17", dict(n_thrs=17)), ("n_areas 0", dict(n_areas=0)), ("n_areas 5", dict(n_areas=5)),
        ("gt area nan", dict(gt_area=_with(a["gt_area"], 1, np.nan))), ("gt area inf", dict(gt_area=_with(a["gt_area"], 0, np.inf))),
        ("gt area negative", dict(gt_area=_with(a["gt_area"], 0, -1.0))),
        ("gt bbox inf", dict(gt_bbox=_with(a["gt_bbox"], (1, 2), -np.inf))), ("gt bbox nan", dict(gt_bbox=_with(a["gt_bbox"], (0, 0), np.nan))),
        ("thr nan", dict(thrs=_with(a["thrs"], 3, np.nan))), ("range inf", dict(rng=_with(a["rng"], (2, 1), np.inf))),
        ("sigma nan", dict(sig=_with(a["sig"], 16, np.nan))), ("sigma zero", dict(sig=_with(a["sig"], 2, 0.0))),
        ("negative n_frames", dict(n=-1)),
    ]
    for what, repl in bad:
        assert c.host(**repl) == lib.OP_ERR_INVALID, what
        assert lib.last_error().startswith("op_keypoint_match: "), (what, lib.last_error())
        assert c.untouched(), what
    # 129 ground truths in frame 1: the message names the frame
    G = 129
    big = dict(gt_off=np.array([0, 0, G], np.int32), gt_kpts=np.zeros((G, 17, 3)), gt_area=np.ones(G), gt_bbox=np.ones((G, 4)),
               gt_ignore=np.zeros(G, np.uint8), gt_crowd=np.zeros(G, np.uint8), oks=np.full(20 * G, 77.0),
               gt_match=np.full(30 * G, 77, np.int32), gt_ig=np.full(3 * G, 77, np.uint8))
    assert c.host(**big) == lib.OP_ERR_INVALID and "frame 1" in lib.last_error() and "128" in lib.last_error()
    with pytest.raises(ValueError, match="frame 0"):
        lib.keypoint_match([(np.zeros((0, 17, 3)), np.zeros(0))], [cases.tables(np.zeros((G, 17, 3)), np.ones(G))])
    with pytest.raises(ValueError, match="max_dets"):
        lib.keypoint_match([], [], max_dets=65)
    assert c.host(n=0) == lib.OP_OK and c.untouched()
    assert c.host() == lib.OP_OK and not c.untouched()


def test_refusals_of_the_staged_entry(lib, K, pd, staged):
    c = _Call(lib, K)
    ctx = staged["ctx"]
    fresh = lib.Context(0)
    try:
        assert c.staged(fresh, 0, 2) == lib.OP_ERR_STATE and "no staged frames" in lib.last_error()
        fresh.stage_frames(FRAMES[:2])  # staged, but no run has left results
        assert c.staged(fresh, 0, 2) == lib.OP_ERR_STATE and "no results" in lib.last_error()
    finally:
        fresh.close()
    for first, n in ((2, 2), (3, 1), (-1, 2), (0, 0), (0, 4)):
        assert c.staged(ctx, first, n) == lib.OP_ERR_INVALID, (first, n)
    a = c.a
    bad = [
        ("null joint_map", dict(joint_map=None)), ("joint 18", dict(joint_map=_with(c.joint_map, 5, 18))),
        ("joint -1", dict(joint_map=_with(c.joint_map, 0, -1))),
        ("null gt_offsets", dict(gt_off=None)), ("null gt table", dict(gt_kpts=None)), ("null thrs", dict(thrs=None)),
        ("null output", dict(status=None)), ("null output", dict(count=None)), ("null output", dict(scores=None)),
        ("null output", dict(dt_order=None)), ("null output", dict(gt_match=None)),
        ("gt offsets decrease", dict(gt_off=np.array([0, a["gt_off"][2], a["gt_off"][1]], np.int32))),
        ("max_dets 65", dict(max_dets=65)), ("n_thrs 17", dict(n_thrs=17)), ("n_areas 5", dict(n_areas=5)),
        ("gt area nan", dict(gt_area=_with(a["gt_area"], 1, np.nan))), ("gt bbox inf", dict(gt_bbox=_with(a["gt_bbox"], (1, 2), np.inf))),
        ("thr inf", dict(thrs=_with(a["thrs"], 0, np.inf))), ("range nan", dict(rng=_with(a["rng"], (0, 0), np.nan))),
    ]
    for what, repl in bad:
        assert c.staged(ctx, 0, 2, **repl) == lib.OP_ERR_INVALID, what
        assert lib.last_error().startswith("op_keypoint_match_staged: "), (what, lib.last_error())
    assert c.staged(None, 0, 2) == lib.OP_ERR_INVALID
    assert c.untouched()
    with pytest.raises(ValueError):
        ctx.keypoint_match(0, 3, staged["gts"][:2])
    assert c.staged(ctx, 0, 2) == lib.OP_OK and not c.untouched()
    assert list(c.extra["status"]) == [lib.OP_OK] * 2 and list(c.extra["count"]) == [7, 0]
    ms = ctypes.c_double()
    assert lib.lib().op_keypoint_last_ms(0, ctypes.byref(ms)) == lib.OP_OK and ms.value > 0
