"""COCO keypoint AP / AR (object keypoint similarity) of detected poses, on the device.

The NumPy functions here (``exp_np``, ``oks_np``, ``match_np``, ``accumulate_np``, ``summarize``)
are the statement: ``COCOeval`` for ``iouType = 'keypoints'`` (``computeOks``, ``evaluateImg``,
``accumulate``, ``summarize``, with ``loadRes``' detection area) restated as recalled, one rounded
IEEE double operation at a time, with no pycocotools and no SciPy.  **Parity unpinned against
pycocotools**: pycocotools is not available where this tree is built and tested, so no number here
has been compared with its output; the statement is the contract, and fixtures made by pycocotools
would belong under tests/golden/ as data.

The device kernel (csrc/keypoint.hip; ``_lib.keypoint_match`` for host data,
``Context.keypoint_match`` for the result rows of a staged batch where the post-process left them)
equals ``match_np`` bit for bit on every output, the OKS matrix included: the statement owns its
exponential (``exp_np``) so that the kernel can repeat it operation by operation.  Accumulation
over a dataset (one sort of all detections per area range) stays on the host.

``evaluate`` / ``evaluate_staged`` are the device entries, ``evaluate_np`` the whole measure on the
host; ``python -m <package>.eval_coco`` is the command line.
"""
import json
import math

import numpy as np

from . import _lib
from .labels import train_params
from .wholebody import pairwise_sum

KPT_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
OKS_THRS = np.linspace(.5, .95, 10)
AREA_RNG = [[0, 1e10], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]
AREA_NAMES = ("all", "medium", "large")
MAX_DETS = 20
REC_THRS = np.linspace(0, 1, 101)
N_KPTS = 17

# exp_np: e^x = 2^k e^r, k = rint(x log2 e), r = x - k ln 2 in two pieces, e^r by its Taylor series
LOG2E = 1.4426950408889634
LN2_HI = 6.93147180369123816490e-01
LN2_LO = 1.90821492927058770002e-10
EXP_COEF = tuple(1.0 / math.factorial(i) for i in range(13, -1, -1))  # 1/13!, ..., 1/1!, 1/0!
EXP_MIN = -708.0


def joint_map():
    """The 17 JointType indices of COCO's keypoints in annotation order (the Neck dropped)."""
    return np.array([int(j) for j in train_params["coco_joint_indices"]], np.int32)


def to_coco(poses18):
    """(P, 18, 3) detector poses -> (P, 17, 3) float64 in COCO's keypoint order: row i is
    ``poses18[:, coco_joint_indices[i]]``, the inverse of ``labels.parse_coco_annotation`` with the
    Neck dropped.  Coordinates stay the detector's doubles, unrounded; a joint that was not found
    stays (0, 0, 0), which is what a COCO results file holds for OpenPose output and what
    ``loadRes`` and ``computeOks`` then see."""
    poses18 = np.asarray(poses18, np.float64).reshape(-1, _lib.N_JOINTS, 3)
    return np.ascontiguousarray(poses18[:, joint_map()])


def results_json(image_id, poses18, scores):
    """The COCO results entries of one image: [{"image_id", "category_id": 1, "keypoints": [51
    numbers], "score"}]."""
    kp = to_coco(poses18)
    return [{"image_id": image_id, "category_id": 1, "keypoints": [float(v) for v in k.ravel()], "score": float(s)}
            for k, s in zip(kp, np.asarray(scores, np.float64).ravel())]


def load_results(path):
    """A COCO keypoint results file -> {image_id: (kpts (D, 17, 3) f64, scores (D,) f64)}, the
    entries of an image in file order (``results_json``'s inverse)."""
    with open(path) as f:
        entries = json.load(f)
    by_image = {}
    for e in entries:
        if e.get("category_id", 1) != 1:
            continue
        by_image.setdefault(e["image_id"], []).append(e)
    return {k: (np.array([e["keypoints"] for e in v], np.float64).reshape(-1, N_KPTS, 3),
                np.array([e["score"] for e in v], np.float64)) for k, v in by_image.items()}


def exp_np(x):
    """e^x for x <= 0 from f64 operations that each round once and exist identically on the device:
    k = rint(x * LOG2E); r = (x - k * LN2_HI) - k * LN2_LO; Horner over 1/13! .. 1/0! written
    p = p * r + c (the multiply and the add round separately); ldexp(p, k).  Below -708 (where
    ``np.exp`` gives a subnormal), and for a NaN, 0.0."""
    x = np.asarray(x, np.float64)
    ok = x >= EXP_MIN
    xs = np.where(ok, x, 0.0)
    k = np.rint(xs * LOG2E)
    r = (xs - k * LN2_HI) - k * LN2_LO
    p = np.full(xs.shape, EXP_COEF[0], np.float64)
    for c in EXP_COEF[1:]:
        p = p * r
        p = p + c
    return np.where(ok, np.ldexp(p, k.astype(np.int32)), 0.0)


def oks_np(dt_kpts, gt_kpts, gt_area, gt_bbox, sigmas=KPT_SIGMAS):
    """``computeOks``: dt_kpts (D, 17, 3), gt_kpts (G, 17, 3), gt_area (G,), gt_bbox (G, 4) as
    (x, y, w, h) -> (D, G) float64.  var = (sigmas * 2) ** 2; with visible gt joints (k1 > 0)
    d = dt - gt on those joints, else the distance to the gt box doubled about its centre on all 17;
    e = (dx*dx + dy*dy) / var / (area + spacing(1)) / 2; oks = pairwise_sum(exp_np(-e)) / count."""
    dt = np.asarray(dt_kpts, np.float64).reshape(-1, N_KPTS, 3)
    gt = np.asarray(gt_kpts, np.float64).reshape(-1, N_KPTS, 3)
    area = np.asarray(gt_area, np.float64).reshape(-1)
    bbox = np.asarray(gt_bbox, np.float64).reshape(-1, 4)
    s2 = np.asarray(sigmas, np.float64) * 2
    var = s2 * s2
    out = np.zeros((len(dt), len(gt)), np.float64)
    if not len(dt):
        return out
    xd, yd = dt[:, :, 0], dt[:, :, 1]
    with np.errstate(all="ignore"):
        for g in range(len(gt)):
            xg, yg, vis = gt[g, :, 0], gt[g, :, 1], gt[g, :, 2] > 0
            k1 = int(np.count_nonzero(vis))
            if k1 > 0:
                dx = xd - xg
                dy = yd - yg
            else:
                bx, by, bw, bh = bbox[g]
                x0, x1 = bx - bw, bx + bw * 2
                y0, y1 = by - bh, by + bh * 2
                dx = np.maximum(0.0, x0 - xd) + np.maximum(0.0, xd - x1)
                dy = np.maximum(0.0, y0 - yd) + np.maximum(0.0, yd - y1)
            e = (dx * dx + dy * dy) / var / (area[g] + np.spacing(1)) / 2
            terms = exp_np(-e)
            if k1 > 0:
                terms = terms[:, vis]
            count = np.float64(terms.shape[1])
            for d in range(len(dt)):
                out[d, g] = pairwise_sum(terms[d]) / count
    return out


def _score_keys(scores):
    s = np.asarray(scores, np.float64).reshape(-1)
    return np.where(np.isnan(s), -np.inf, s)


def dt_areas(dt_kpts):
    """``loadRes``' area of a keypoint detection: (max x - min x) * (max y - min y) over all 17
    rows, zeros included."""
    dt = np.asarray(dt_kpts, np.float64).reshape(-1, N_KPTS, 3)
    if not len(dt):
        return np.zeros(0, np.float64)
    with np.errstate(all="ignore"):
        x, y = dt[:, :, 0], dt[:, :, 1]
        return (x.max(axis=1) - x.min(axis=1)) * (y.max(axis=1) - y.min(axis=1))


def match_np(dt_kpts, dt_scores, gt_kpts, gt_area, gt_bbox, gt_ignore, gt_iscrowd, max_dets=MAX_DETS,
             thrs=OKS_THRS, area_rng=AREA_RNG, sigmas=KPT_SIGMAS):
    """``evaluateImg`` of one image for every area range and threshold -> a dict:

        dt_order  (D',)       the detections kept, by descending score (stable; NaN as -inf), cut to max_dets
        dt_scores (D',)       their scores
        oks       (D', G)     rows in dt_order, columns in the caller's gt order
        dt_match  (A, T, D')  int32 gt index (caller's order), -1 for none
        dt_ignore (A, T, D')  uint8
        gt_match  (A, T, G)   int32 detection index (caller's order), -1 for none
        gt_ignore (A, G)      uint8: gt_ignore[g] or the gt's area outside the range
    """
    dt = np.asarray(dt_kpts, np.float64).reshape(-1, N_KPTS, 3)
    scores = np.asarray(dt_scores, np.float64).reshape(-1)
    gt = np.asarray(gt_kpts, np.float64).reshape(-1, N_KPTS, 3)
    area = np.asarray(gt_area, np.float64).reshape(-1)
    ign = np.asarray(gt_ignore).reshape(-1).astype(bool)
    crowd = np.asarray(gt_iscrowd).reshape(-1).astype(bool)
    thrs = np.asarray(thrs, np.float64).reshape(-1)
    rng = np.asarray(area_rng, np.float64).reshape(-1, 2)
    order = np.argsort(-_score_keys(scores), kind="mergesort")[:int(max_dets)].astype(np.int32)
    dt = dt[order]
    D, G, A, T = len(dt), len(gt), len(rng), len(thrs)
    oks = oks_np(dt, gt, area, gt_bbox, sigmas)
    d_area = dt_areas(dt)
    dt_match = np.full((A, T, D), -1, np.int32)
    dt_ignore = np.zeros((A, T, D), np.uint8)
    gt_match = np.full((A, T, G), -1, np.int32)
    gt_ig = np.zeros((A, G), np.uint8)
    for a, (lo, hi) in enumerate(rng):
        ig = np.array([bool(ign[g]) or bool(area[g] < lo) or bool(area[g] > hi) for g in range(G)], bool)
        gt_ig[a] = ig
        visit = [int(g) for g in np.argsort(ig, kind="mergesort")]  # not ignored first, stably
        for t, thr in enumerate(thrs):
            matched = [False] * G
            for d in range(D):
                bound = min(float(thr), 1 - 1e-10)
                m = -1
                for g in visit:
                    if matched[g] and not crowd[g]:
                        continue
                    if m > -1 and not ig[m] and ig[g]:
                        break
                    if oks[d, g] < bound:
                        continue
                    bound = oks[d, g]
                    m = g
                if m > -1:
                    dt_ignore[a, t, d] = ig[m]
                    dt_match[a, t, d] = m
                    gt_match[a, t, m] = order[d]
                    matched[m] = True
                elif d_area[d] < lo or d_area[d] > hi:
                    dt_ignore[a, t, d] = 1
    return {"dt_order": order, "dt_scores": scores[order], "oks": oks, "dt_match": dt_match, "dt_ignore": dt_ignore,
            "gt_match": gt_match, "gt_ignore": gt_ig}


def accumulate_np(per_image, n_areas=len(AREA_RNG), n_thrs=len(OKS_THRS), rec_thrs=REC_THRS):
    """``accumulate`` for one category and one maxDets over ``match_np``'s records (one per image;
    images with neither detections nor ground truths are left out) -> {"precision" (T, R, A),
    "recall" (T, A)}, -1 where an area range has no ground truth that counts."""
    rec_thrs = np.asarray(rec_thrs, np.float64)
    A, T, R = int(n_areas), int(n_thrs), len(rec_thrs)
    precision = -np.ones((T, R, A))
    recall = -np.ones((T, A))
    images = [r for r in per_image if len(r["dt_scores"]) or r["gt_ignore"].shape[1]]
    if not images:
        return {"precision": precision, "recall": recall}
    keys = _score_keys(np.concatenate([r["dt_scores"] for r in images]))
    inds = np.argsort(-keys, kind="mergesort")
    for a in range(A):
        dtm = np.concatenate([r["dt_match"][a].reshape(T, -1) for r in images], axis=1)[:, inds]
        dtig = np.concatenate([r["dt_ignore"][a].reshape(T, -1) for r in images], axis=1)[:, inds].astype(bool)
        gtig = np.concatenate([r["gt_ignore"][a] for r in images])
        npig = int(np.count_nonzero(gtig == 0))
        if npig == 0:
            continue
        tps = np.logical_and(dtm >= 0, np.logical_not(dtig))
        fps = np.logical_and(dtm < 0, np.logical_not(dtig))
        tp_sum = np.cumsum(tps, axis=1).astype(np.float64)
        fp_sum = np.cumsum(fps, axis=1).astype(np.float64)
        for t in range(T):
            tp, fp = tp_sum[t], fp_sum[t]
            nd = len(tp)
            rc = tp / npig
            pr = tp / (fp + tp + np.spacing(1))
            recall[t, a] = rc[-1] if nd else 0
            pr = pr.tolist()
            for i in range(nd - 1, 0, -1):
                if pr[i] > pr[i - 1]:
                    pr[i - 1] = pr[i]
            q = np.zeros(R)
            for ri, pi in enumerate(np.searchsorted(rc, rec_thrs, side="left")):
                if pi >= nd:
                    break
                q[ri] = pr[pi]
            precision[t, :, a] = q
    return {"precision": precision, "recall": recall}


def summarize(acc, thrs=OKS_THRS):
    """``summarize``'s ten numbers in COCOeval's order: AP, AP50, AP75, APm, APl, AR, AR50, AR75,
    ARm, ARl; each the mean of the entries above -1, or -1 when there are none."""
    thrs = np.asarray(thrs, np.float64)

    def mean(s):
        s = s[s > -1]
        return float(np.mean(s)) if len(s) else -1.0

    def stat(ap, thr=None, area=0):
        s = acc["precision"] if ap else acc["recall"]
        if thr is not None:
            s = s[np.where(np.isclose(thrs, thr))[0]]
        return mean(s[..., area])

    return np.array([stat(1), stat(1, .5), stat(1, .75), stat(1, area=1), stat(1, area=2),
                     stat(0), stat(0, .5), stat(0, .75), stat(0, area=1), stat(0, area=2)])


def format_summary(stats, max_dets=MAX_DETS):
    """COCOeval's ten summary lines."""
    rows = [(1, None, "all"), (1, .5, "all"), (1, .75, "all"), (1, None, "medium"), (1, None, "large"),
            (0, None, "all"), (0, .5, "all"), (0, .75, "all"), (0, None, "medium"), (0, None, "large")]
    lines = []
    for (ap, thr, area), v in zip(rows, stats):
        title, kind = ("Average Precision", "(AP)") if ap else ("Average Recall", "(AR)")
        iou = "%0.2f:%0.2f" % (OKS_THRS[0], OKS_THRS[-1]) if thr is None else "%0.2f" % thr
        lines.append(" {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}".format(
            title, kind, iou, area, int(max_dets), float(v)))
    return lines


def gt_tables(annotations):
    """The person annotations of one image (plain dicts; every ``category_id == 1`` one takes part,
    not only those ``labels.valid_annotations`` keeps) -> (kpts (G, 17, 3) f64, area (G,), bbox
    (G, 4), ignore (G,) uint8 = iscrowd or num_keypoints == 0, iscrowd (G,) uint8)."""
    anns = [a for a in annotations if a.get("category_id", 1) == 1]
    G = len(anns)
    kpts = np.zeros((G, N_KPTS, 3), np.float64)
    area = np.zeros(G, np.float64)
    bbox = np.zeros((G, 4), np.float64)
    ignore = np.zeros(G, np.uint8)
    crowd = np.zeros(G, np.uint8)
    for g, a in enumerate(anns):
        kpts[g] = np.asarray(a["keypoints"], np.float64).reshape(N_KPTS, 3)
        area[g] = a["area"]
        bbox[g] = a["bbox"]
        crowd[g] = 1 if a.get("iscrowd", 0) else 0
        nk = a["num_keypoints"] if "num_keypoints" in a else int(np.count_nonzero(kpts[g, :, 2] > 0))
        ignore[g] = 1 if (crowd[g] or nk == 0) else 0
    return kpts, area, bbox, ignore, crowd


def _result(per_image):
    acc = accumulate_np(per_image)
    acc["stats"] = summarize(acc)
    return acc


def evaluate_np(dets_per_image, gts_per_image):
    """The whole measure on the host.  dets_per_image: per image (kpts (D, 17, 3), scores (D,));
    gts_per_image: per image ``gt_tables``' tuple -> {"precision", "recall", "stats" (10,)}."""
    if len(dets_per_image) != len(gts_per_image):
        raise ValueError("evaluate_np: %d images of detections, %d of ground truths" % (len(dets_per_image), len(gts_per_image)))
    return _result([match_np(k, s, *gt) for (k, s), gt in zip(dets_per_image, gts_per_image)])


def evaluate(dets_per_image, gts_per_image, device=0):
    """``evaluate_np`` with the matching on the device (one ``_lib.keypoint_match`` call for all
    images, the OKS matrices left there) and the accumulation on the host: the same dict."""
    if len(dets_per_image) != len(gts_per_image):
        raise ValueError("evaluate: %d images of detections, %d of ground truths" % (len(dets_per_image), len(gts_per_image)))
    return _result(_lib.keypoint_match(dets_per_image, gts_per_image, device=device, want_oks=False))


def evaluate_staged(pose_detector, first, n, gts, max_dets=MAX_DETS, want_oks=False):
    """The per-image match records (``match_np``'s dict, ``oks`` only when asked for) of staged
    frames [first, first + n) of ``pose_detector``'s context after its staged run, ``gts`` their
    ``gt_tables``: one ``Context.keypoint_match`` call reads the result rows where they lie; only
    the ground-truth tables go up and only the match block comes back.  The records are ready for
    ``accumulate_np``, so a dataset of many batches accumulates once at the end.  A frame over the
    batched post-process caps is taken through ``fetch_result`` and ``_lib.keypoint_match``; one on
    which the reference's grouping raises IndexError (pose_detector.py:197) raises it here too."""
    ctx = pose_detector.staged_context()
    first, n = int(first), int(n)
    status, records = ctx.keypoint_match(first, n, gts, joint_map=joint_map(), max_dets=max_dets, want_oks=want_oks)
    for i in range(n):
        if status[i] != _lib.OP_OK:
            poses, scores, _ = ctx.fetch_result(first + i)
            records[i] = _lib.keypoint_match([(to_coco(poses), scores)], [gts[i]], device=pose_detector.device,
                                             max_dets=max_dets, want_oks=want_oks)[0]
    return records
