"""keypoint_eval's NumPy statement of the COCO keypoint measure, on the host: its exponential
against ``np.exp``, the OKS arithmetic on hand cases, ``match_np`` against a second, naive matcher
on the case set, ``accumulate_np`` / ``summarize`` on hand-computed cases, and the round trips."""
import json

import numpy as np
import pytest

import keypoint_cases as cases
from conftest import pkg_module


@pytest.fixture(scope="module")
def K():
    return pkg_module("keypoint_eval")


def _ulps(a, b):
    return np.abs(np.ascontiguousarray(a, np.float64).view(np.int64) - np.ascontiguousarray(b, np.float64).view(np.int64))


def test_exp_np_within_one_ulp_of_np_exp(K):
    rng = np.random.default_rng(11)
    x = np.concatenate([rng.uniform(-708.0, 0.0, 700000),
                        -np.exp(rng.uniform(np.log(1e-300), np.log(708.0), 400000)),  # dense near 0
                        [-708.0, -1e-320, -0.5, -1.0, -np.log(2.0)]])
    d = _ulps(K.exp_np(x), np.exp(x))
    print("exp_np: %d points, max %d ulp, %.1f %% equal" % (len(x), d.max(), 100.0 * (d == 0).mean()))
    assert len(x) >= 1000000 and d.max() <= 1
    assert K.exp_np(0.0) == 1.0 and K.exp_np(-0.0) == 1.0
    assert K.exp_np(np.nextafter(-708.0, -1e9)) == 0.0 and K.exp_np(-1e5) == 0.0 and K.exp_np(-np.inf) == 0.0
    assert K.exp_np(np.array([0.0, -800.0])).tolist() == [1.0, 0.0]


def test_oks_one_visible_joint(K):
    for joint, d, area in ((0, 3.0, 900.0), (5, 12.5, 4000.0), (16, 0.25, 77.0)):
        gt = np.zeros((1, 17, 3))
        gt[0, joint] = (50.0, 60.0, 2.0)
        dt = np.full((1, 17, 3), 7.0)
        dt[0, joint] = (50.0 + d, 60.0, 1.0)
        got = K.oks_np(dt, gt, [area], [[0, 0, 10, 10]])[0, 0]
        want = np.exp(-d * d / (2 * area * (2 * K.KPT_SIGMAS[joint]) ** 2))
        assert abs(got - want) <= 1e-15 * want, (joint, got, want)


def test_oks_coincident_and_box_cases(K):
    rng = np.random.default_rng(3)
    gt = cases.person(rng, 100, 100, 50.0, 11)
    dt = gt.copy()
    dt[:, 2] = 1.0
    assert K.oks_np(dt[None], gt[None], [1200.0], [[75, 75, 50, 50]])[0, 0] == 1.0
    # k1 == 0: distance to the box doubled about itself (x 120 .. 360, y 50 .. 350)
    g0 = np.zeros((1, 17, 3))
    box = [[200.0, 150.0, 80.0, 100.0]]
    inside = cases.person(rng, 240, 200, 100.0)
    corners = inside.copy()
    corners[:, 0], corners[:, 1] = np.where(np.arange(17) % 2, 120.0, 360.0), np.where(np.arange(17) % 3, 50.0, 350.0)
    outside = inside.copy()
    outside[4, 0] = 361.0
    oks = K.oks_np(np.array([inside, corners, outside]), g0, [6400.0], box)[:, 0]
    assert oks[0] == 1.0 and oks[1] == 1.0 and 0.0 < oks[2] < 1.0
    want = (16 + np.exp(-1.0 / (2 * 6400.0 * (2 * K.KPT_SIGMAS[4]) ** 2))) / 17
    assert abs(oks[2] - want) <= 4e-16


def naive_match(K, dets, gts, max_dets):
    """evaluateImg the way COCOeval writes it: ground truths re-ordered "not ignored first", the
    search in that order's index space, matches as 1-based ids with 0 for none, mapped back after."""
    kp, scores = dets
    gk, area, bbox, ignore, crowd = gts
    keys = [(-np.inf if np.isnan(s) else s) for s in scores]
    order = sorted(range(len(keys)), key=lambda i: -keys[i])[:max_dets]  # sorted() is stable
    oks_all = K.oks_np(kp[order], gk, area, bbox)
    d_area = [(k[:, 0].max() - k[:, 0].min()) * (k[:, 1].max() - k[:, 1].min()) for k in kp[order]]
    A, T, D, G = len(K.AREA_RNG), len(K.OKS_THRS), len(order), len(gk)
    out = {"dt_match": -np.ones((A, T, D), np.int32), "dt_ignore": np.zeros((A, T, D), np.uint8),
           "gt_match": -np.ones((A, T, G), np.int32), "gt_ignore": np.zeros((A, G), np.uint8),
           "dt_order": np.array(order, np.int32), "oks": oks_all}
    for a, (lo, hi) in enumerate(K.AREA_RNG):
        flags = [1 if (ignore[g] or area[g] < lo or area[g] > hi) else 0 for g in range(G)]
        gtind = [g for g in range(G) if not flags[g]] + [g for g in range(G) if flags[g]]
        gt_ig = [flags[g] for g in gtind]
        is_crowd = [int(crowd[g]) for g in gtind]
        ious = oks_all[:, gtind] if G else oks_all
        gtm = np.zeros((T, G), np.int64)
        dtm = np.zeros((T, D), np.int64)
        dt_ig = np.zeros((T, D), np.int64)
        for tind, t in enumerate(K.OKS_THRS):
            for dind in range(D):
                iou = min([t, 1 - 1e-10])
                m = -1
                for gind in range(G):
                    if gtm[tind, gind] > 0 and not is_crowd[gind]:
                        continue
                    if m > -1 and gt_ig[m] == 0 and gt_ig[gind] == 1:
                        break
                    if ious[dind, gind] < iou:
                        continue
                    iou = ious[dind, gind]
                    m = gind
                if m == -1:
                    continue
                dt_ig[tind, dind] = gt_ig[m]
                dtm[tind, dind] = gtind[m] + 1
                gtm[tind, m] = order[dind] + 1
        outside = np.array([a_ < lo or a_ > hi for a_ in d_area], bool).reshape(1, D)
        dt_ig = np.logical_or(dt_ig, np.logical_and(dtm == 0, np.repeat(outside, T, 0)))
        out["dt_match"][a] = dtm - 1
        out["dt_ignore"][a] = dt_ig
        for pos, g in enumerate(gtind):
            out["gt_match"][a][:, g] = gtm[:, pos] - 1
        out["gt_ignore"][a] = flags
    return out


def test_match_np_equals_a_naive_matcher_on_the_case_set(K):
    frames, refs = cases.all_frames(), cases.references(K)
    assert len(frames) >= 48
    seen = {"matched": 0, "ignored": 0, "crowd_twice": 0}
    for (name, dets, gts), ref in zip(frames, refs):
        want = naive_match(K, dets, gts, cases.MAX_DETS)
        for key, val in want.items():
            assert ref[key].shape == val.shape and np.array_equal(ref[key], val), (name, key)
        seen["matched"] += int((ref["dt_match"] >= 0).sum())
        seen["ignored"] += int(ref["dt_ignore"].sum())
        if name == "crowd_matched_by_two_detections":
            seen["crowd_twice"] = int(((ref["dt_match"][0] == 0).sum(axis=1) == 2).sum())
    assert seen["matched"] > 1000 and seen["ignored"] > 100 and seen["crowd_twice"] >= 1, seen
    by = {name: ref for (name, _, _), ref in zip(frames, refs)}
    assert len(by["25_detections_cut_to_20"]["dt_order"]) == 20 and by["128_ground_truths_the_cap"]["oks"].shape == (20, 128)
    assert by["tied_scores"]["dt_order"].tolist() == [1, 3, 6, 0, 2, 4, 5, 7]
    assert by["nan_score"]["dt_order"].tolist() == [2, 0, 4, 1, 3]
    assert by["e_above_708"]["oks"][1, 0] == 0.0 and by["e_above_708"]["oks"][0, 0] > 0.5
    oks = by["ground_truth_without_keypoints"]["oks"][:, 0]
    assert oks[0] == 1.0 and oks[1] == 1.0 and 0 < oks[2] < 1 and oks[3] < oks[2]


def _records(K, dt_match, dt_ignore, gt_ignore, scores):
    """One image's record from (T, D) / (G,) rows repeated over the three area ranges."""
    A = len(K.AREA_RNG)
    dt_match = np.asarray(dt_match, np.int32)
    return {"dt_scores": np.asarray(scores, np.float64), "dt_match": np.repeat(dt_match[None], A, 0),
            "dt_ignore": np.repeat(np.asarray(dt_ignore, np.uint8)[None], A, 0),
            "gt_ignore": np.repeat(np.asarray(gt_ignore, np.uint8)[None], A, 0)}


def _gt_of(rng, n, size):
    kp = np.array([cases.person(rng, 100 + 150 * i, 200, size, 17) for i in range(n)])
    return cases.tables(kp, [size * size / 2.0] * n)


def test_perfect_detections(K):
    rng = np.random.default_rng(8)
    gts = [_gt_of(rng, 3, 100.0), _gt_of(rng, 2, 120.0)]  # areas 5000 and 7200: medium only
    dets = [(g[0].copy(), np.arange(len(g[0]), 0, -1.0)) for g in gts]
    stats = K.evaluate_np(dets, gts)["stats"]
    assert np.abs(stats[[0, 1, 2, 3, 5, 6, 7, 8]] - 1).max() <= 1e-12
    assert stats[4] == -1 and stats[9] == -1
    lines = K.format_summary(stats)
    assert lines[0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets= 20 ] = 1.000"
    assert lines[9] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets= 20 ] = -1.000"
    assert lines[6] == " Average Recall     (AR) @[ IoU=0.50      | area=   all | maxDets= 20 ] = 1.000"


def test_no_detections(K):
    rng = np.random.default_rng(8)
    gts = [_gt_of(rng, 3, 100.0)]
    stats = K.evaluate_np([(np.zeros((0, 17, 3)), np.zeros(0))], gts)["stats"]
    assert stats[0] == 0 and stats[5] == 0 and stats[3] == 0 and stats[4] == -1


def test_tp_fp_tp_by_score(K):
    T = len(K.OKS_THRS)
    rec = _records(K, np.repeat([[0, -1, 1]], T, 0), np.zeros((T, 3)), [0, 0], [0.9, 0.8, 0.7])
    acc = K.accumulate_np([rec])
    want = (51 + 50 * 2.0 / 3.0) / 101
    assert np.allclose(acc["recall"], 1.0, rtol=0, atol=0)
    p = acc["precision"][0, :, 0]
    assert np.allclose(p[:51], 1.0, rtol=0, atol=1e-15) and np.allclose(p[51:], 2.0 / 3.0, rtol=0, atol=1e-15)
    assert abs(K.summarize(acc)[0] - want) <= 1e-12 and abs(K.summarize(acc)[1] - want) <= 1e-12
    # the same three detections spread over two images, given in another order
    a = _records(K, np.repeat([[-1]], T, 0), np.zeros((T, 1)), [0], [0.8])
    b = _records(K, np.repeat([[0, 1]], T, 0), np.zeros((T, 2)), [0], [0.9, 0.7])
    b["dt_match"][:, :, 1] = -1  # image b: TP at 0.9, FP at 0.7; image a: FP at 0.8 -> TP FP FP
    acc2 = K.accumulate_np([a, b])
    assert np.allclose(acc2["recall"], 0.5, rtol=0, atol=0)
    assert abs(K.summarize(acc2)[0] - 51.0 / 101) <= 1e-12


def test_crowd_absorbs_two_detections(K):
    rng = np.random.default_rng(9)
    g_crowd, g_one = cases.person(rng, 300, 200, 150.0, 10), cases.person(rng, 80, 80, 60.0, 15)
    dt = np.array([g_crowd, g_crowd + [0.5, 0.5, 0], g_one])
    gts = cases.tables([g_crowd, g_one], [150.0 ** 2 / 2, 60.0 ** 2 / 2], crowd=[1, 0])
    rec = K.match_np(dt, [9.0, 8.0, 7.0], *gts)
    assert (rec["dt_match"][0, 0] == [0, 0, 1]).all() and (rec["dt_ignore"][0, 0] == [1, 1, 0]).all()
    stats = K.evaluate_np([(dt, [9.0, 8.0, 7.0])], [gts])["stats"]
    assert abs(stats[0] - 1) <= 1e-12 and abs(stats[5] - 1) <= 1e-12  # neither crowd match is a false positive


def test_detection_on_out_of_range_ground_truth(K):
    rng = np.random.default_rng(10)
    small, mid = cases.person(rng, 100, 100, 30.0, 17), cases.person(rng, 300, 300, 90.0, 17)
    gts = cases.tables([small, mid], [500.0, 4000.0])  # small: below 32^2, outside medium
    dt = np.array([small, mid])
    rec = K.match_np(dt, [2.0, 1.0], *gts)
    assert rec["gt_ignore"].tolist() == [[0, 0], [1, 0], [1, 1]]
    assert rec["dt_match"][0, 0].tolist() == [0, 1] and rec["dt_ignore"][0, 0].tolist() == [0, 0]
    assert rec["dt_match"][1, 0].tolist() == [0, 1] and rec["dt_ignore"][1, 0].tolist() == [1, 0]
    acc = K.accumulate_np([rec])
    assert acc["recall"][0, 0] == 1.0 and acc["recall"][0, 1] == 1.0 and acc["recall"][0, 2] == -1


def test_host_entry_refuses_before_any_device_call(lib, K):
    """op_keypoint_match validates on the host first: these are refused (OP_ERR_INVALID, the frame
    named) whether or not there is a device; tests/test_gpu_keypoint_eval.py has the whole list."""
    none = (np.zeros((0, 17, 3)), np.zeros(0))
    g129 = cases.tables(np.zeros((129, 17, 3)), np.ones(129))
    g1 = cases.tables(np.zeros((1, 17, 3)), [np.nan])
    with pytest.raises(ValueError, match="gt_offsets: frame 1: 129 ground truths, at most 128 per frame"):
        lib.keypoint_match([none, none], [cases.tables(np.zeros((0, 17, 3)), []), g129])
    with pytest.raises(ValueError, match="gt_area: frame 0"):
        lib.keypoint_match([none], [g1])
    with pytest.raises(ValueError, match="n_thrs"):
        lib.keypoint_match([none], [g1], thrs=np.linspace(0.1, 0.9, 17))
    with pytest.raises(ValueError, match="thrs: not finite"):
        lib.keypoint_match([none], [cases.tables(np.zeros((1, 17, 3)), [1.0])], thrs=[0.5, np.inf])
    assert lib.lib().op_keypoint_match(0, 0, *([None] * 9), 20, 10, None, 3, None, None, *([None] * 6)) == lib.OP_OK
    assert lib.lib().op_keypoint_match(0, 1, *([None] * 9), 20, 10, None, 3, None, None, *([None] * 6)) == lib.OP_ERR_INVALID
    assert lib.last_error() == "op_keypoint_match: null dt_offsets"
    assert lib.lib().op_keypoint_match_staged(None, 0, 1, *([None] * 7), 20, 10, None, 3, None, None, *([None] * 9)) == lib.OP_ERR_INVALID
    assert lib.last_error() == "op_keypoint_match_staged: null context"


def test_evaluate_staged_takes_a_frame_over_the_caps_through_the_host_entry(lib, K, monkeypatch):
    """The Python layer alone (no device: the two device calls are stand-ins that answer with the
    statement): a frame whose status is not OP_OK is fetched and matched through the host entry."""
    rng = np.random.default_rng(14)
    poses = rng.uniform(10, 300, (2, 3, 18, 3))
    poses[:, :, :, 2] = 1.0
    scores = rng.uniform(1, 9, (2, 3))
    gts = [cases.tables(K.to_coco(p)[:2] + [1.5, -1.0, 1.0], [5000.0, 7000.0]) for p in poses]
    calls = []

    class Ctx(object):
        def keypoint_match(self, first, n, g, joint_map=None, max_dets=None, want_oks=False):
            assert (first, n) == (4, 2) and list(joint_map) == list(K.joint_map())
            empty = K.match_np(np.zeros((0, 17, 3)), np.zeros(0), *g[1], max_dets=max_dets)
            return np.array([lib.OP_OK, lib.OP_ERR_CAPACITY]), [
                K.match_np(K.to_coco(poses[0]), scores[0], *g[0], max_dets=max_dets), empty]

        def fetch_result(self, frame):
            calls.append(frame)
            return poses[frame - 4], scores[frame - 4], None

    class Det(object):
        device = 0

        def staged_context(self):
            return Ctx()

    def host_entry(dets, g, device=0, max_dets=None, want_oks=True):
        return [K.match_np(k, s, *t, max_dets=max_dets) for (k, s), t in zip(dets, g)]

    monkeypatch.setattr(lib, "keypoint_match", host_entry)
    recs = K.evaluate_staged(Det(), 4, 2, gts)
    assert calls == [5]
    for i in range(2):
        want = K.match_np(K.to_coco(poses[i]), scores[i], *gts[i])
        assert all(np.array_equal(recs[i][k], want[k]) for k in want)
    assert len(recs[1]["dt_order"]) == 3 and (recs[1]["dt_match"] >= 0).any()


def test_round_trips(K, tmp_path):
    labels = pkg_module("labels")
    rng = np.random.default_rng(12)
    anns = []
    for i in range(4):
        kp = cases.person(rng, 200, 150, 120.0, 17 if i == 0 else 9).round()
        anns.append({"keypoints": [int(v) for v in kp.ravel()], "num_keypoints": int((kp[:, 2] > 0).sum()), "area": 4000.0 + i,
                     "bbox": [140.0, 90.0, 120.0, 120.0], "iscrowd": int(i == 3), "category_id": 1, "image_id": 7, "id": i})
    poses18 = labels.parse_coco_annotation(anns)
    want = np.array([a["keypoints"] for a in anns], np.float64).reshape(-1, 17, 3)
    got = K.to_coco(poses18)
    assert got.dtype == np.float64 and np.array_equal(got, want)
    kp, area, bbox, ignore, crowd = K.gt_tables(anns + [{"category_id": 2, "keypoints": [0] * 51, "area": 1, "bbox": [0] * 4}])
    assert np.array_equal(kp, want) and area.tolist() == [4000.0, 4001.0, 4002.0, 4003.0]
    assert ignore.tolist() == [0, 0, 0, 1] and crowd.tolist() == [0, 0, 0, 1] and bbox.shape == (4, 4)
    # results_json -> file -> load_results
    poses = rng.uniform(-5, 700, (3, 18, 3))
    poses[1, 4] = 0.0
    scores = np.array([12.25, 3.0000000000000004, 0.1])
    entries = K.results_json(42, poses, scores) + K.results_json(43, poses[:1], scores[:1])
    path = tmp_path / "results.json"
    path.write_text(json.dumps(entries))
    back = K.load_results(str(path))
    assert sorted(back) == [42, 43]
    assert np.array_equal(back[42][0], K.to_coco(poses)) and np.array_equal(back[42][1], scores)
    assert np.array_equal(back[43][0], K.to_coco(poses[:1])) and len(entries[0]["keypoints"]) == 51
