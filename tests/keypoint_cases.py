"""Frames for the keypoint-evaluation tests (test_keypoint_eval_host.py, test_gpu_keypoint_eval.py):
seeded synthetic images, a few persons each, one named case per property the matcher, the OKS
arithmetic and the ordering can get wrong.  A frame is (name, (dt_kpts (D, 17, 3), dt_scores (D,)),
(gt_kpts (G, 17, 3), gt_area (G,), gt_bbox (G, 4), gt_ignore (G,), gt_iscrowd (G,)))."""
import numpy as np

MAX_DETS = 20


def person(rng, cx, cy, size, visible=17):
    """17 keypoints within a size x size box about (cx, cy); the first ``visible`` of a seeded
    permutation labelled (v = 2), the others (0, 0, 0) as COCO stores them."""
    k = np.zeros((17, 3))
    k[:, 0] = cx + rng.uniform(-0.5, 0.5, 17) * size
    k[:, 1] = cy + rng.uniform(-0.5, 0.5, 17) * size
    k[:, 2] = 2.0
    hide = rng.permutation(17)[visible:]
    k[hide] = 0.0
    return k


def tables(kpts, areas, boxes=None, ignore=None, crowd=None):
    kpts = np.asarray(kpts, np.float64).reshape(-1, 17, 3)
    G = len(kpts)
    areas = np.asarray(areas, np.float64).reshape(-1)
    if boxes is None:
        boxes = np.zeros((G, 4))
        for g in range(G):
            s = np.sqrt(areas[g] * 2.0)
            vis = kpts[g, :, 2] > 0
            c = kpts[g, vis, :2].mean(axis=0) if vis.any() else np.zeros(2)
            boxes[g] = [c[0] - s / 2, c[1] - s / 2, s, s]
    crowd = np.zeros(G, np.uint8) if crowd is None else np.asarray(crowd, np.uint8)
    nk0 = (kpts[:, :, 2] > 0).sum(axis=1) == 0
    ignore = ((crowd != 0) | nk0).astype(np.uint8) if ignore is None else np.asarray(ignore, np.uint8)
    return kpts, areas, np.asarray(boxes, np.float64).reshape(-1, 4), ignore, crowd


def detect(rng, gt, size, noise):
    """A detection of a ground truth: every joint found, ``noise * size`` px off."""
    d = np.array(gt, np.float64)
    miss = d[:, 2] == 0
    d[:, :2] += rng.normal(0.0, noise * size, (17, 2))
    d[miss, :2] = d[~miss, :2].mean(axis=0) + rng.normal(0.0, 0.3 * size, (int(miss.sum()), 2)) if (~miss).any() else 0.0
    d[:, 2] = 1.0
    return d


def scene(rng, G, D, size_range=(20.0, 220.0), visible=None):
    """G ground truths, D detections: detection i sits on ground truth i % G (when there is one)."""
    sizes = rng.uniform(size_range[0], size_range[1], max(G, 1))
    gts = [person(rng, rng.uniform(50, 600), rng.uniform(50, 400), sizes[g],
                  int(rng.integers(1, 18)) if visible is None else visible) for g in range(G)]
    dts = []
    for d in range(D):
        if G:
            g = d % G
            dts.append(detect(rng, gts[g], sizes[g], rng.uniform(0.01, 0.2)))
        else:
            dts.append(detect(rng, person(rng, 300, 200, 80.0), 80.0, 0.05))
    scores = rng.uniform(0.1, 30.0, D)
    areas = sizes[:G] ** 2 * rng.uniform(0.3, 0.7, G)
    return (np.array(dts).reshape(-1, 17, 3), scores), tables(np.array(gts).reshape(-1, 17, 3), areas)


def frames():
    rng = np.random.default_rng(20)
    out = []

    def add(name, dets, gts):
        out.append((name, (np.asarray(dets[0], np.float64).reshape(-1, 17, 3), np.asarray(dets[1], np.float64).reshape(-1)), gts))

    # ---- counts and ordering ----
    add("no_detections", *scene(rng, 3, 0))
    add("no_ground_truths", *scene(rng, 0, 3))
    add("neither", *scene(rng, 0, 0))
    add("25_detections_cut_to_20", *scene(rng, 6, 25))
    add("20_detections_exactly", *scene(rng, 5, 20))
    add("70_ground_truths", *scene(rng, 70, 12))
    add("128_ground_truths_the_cap", *scene(rng, 128, 25))
    dets, gts = scene(rng, 4, 5, visible=12)
    add("every_ground_truth_ignored", dets, gts[:3] + (np.ones(4, np.uint8), gts[4]))
    # a crowd region with two detections on it, beside one ordinary person with one detection
    g_crowd, g_one = person(rng, 300, 200, 150.0, 10), person(rng, 80, 80, 60.0, 15)
    dets = np.array([detect(rng, g_crowd, 150.0, 0.03), detect(rng, g_crowd, 150.0, 0.05), detect(rng, g_one, 60.0, 0.03)])
    add("crowd_matched_by_two_detections", (dets, [9.0, 8.0, 7.0]),
        tables([g_crowd, g_one], [150.0 ** 2 / 2, 60.0 ** 2 / 2], crowd=[1, 0]))
    dets, gts = scene(rng, 4, 8, visible=14)
    add("tied_scores", (dets[0], [3.0, 5.0, 3.0, 5.0, 3.0, 3.0, 5.0, -0.0]), gts)
    dets, gts = scene(rng, 3, 3, visible=14)
    add("duplicated_detection", (np.concatenate([dets[0], dets[0][:2]]), [4.0, 2.0, 6.0, 4.0, 9.0]), gts)
    # ---- arithmetic ----
    # a ground truth without labelled keypoints: OKS from the distance to its doubled box
    g_nk0 = np.zeros((17, 3))
    box = [200.0, 150.0, 80.0, 100.0]  # doubled: x 120 .. 360, y 50 .. 350
    inside = person(rng, 240, 200, 100.0)
    edge = person(rng, 240, 200, 100.0)
    edge[:, 0] = np.linspace(120.0, 360.0, 17)
    outside = person(rng, 420, 400, 90.0)
    far_out = person(rng, -300, 900, 90.0)
    g_p = person(rng, 500, 100, 70.0, 13)
    add("ground_truth_without_keypoints", (np.array([inside, edge, outside, far_out, detect(rng, g_p, 70.0, 0.05)]),
                                           [5.0, 4.0, 3.0, 2.0, 1.0]),
        tables([g_nk0, g_p], [6400.0, 2400.0], boxes=[box, [465.0, 65.0, 70.0, 70.0]]))
    vis = (1, 7, 8, 9, 16, 17)
    gk = [person(rng, 60 + 100 * i, 120 + 20 * i, 80.0, v) for i, v in enumerate(vis)]
    add("1_7_8_9_16_17_visible_joints", (np.array([detect(rng, g, 80.0, 0.06) for g in gk]), rng.uniform(1, 9, 6)),
        tables(gk, [3000.0] * 6))
    edges = [32.0 ** 2, 96.0 ** 2, np.nextafter(32.0 ** 2, 0), np.nextafter(32.0 ** 2, 1e9), np.nextafter(96.0 ** 2, 0),
             np.nextafter(96.0 ** 2, 1e9)]
    sz = [np.sqrt(a * 2) for a in edges]
    gk = [person(rng, 70 + 110 * i, 200.0, sz[i], 15) for i in range(6)]
    add("areas_on_the_range_edges", (np.array([detect(rng, g, s, 0.04) for g, s in zip(gk, sz)]), rng.uniform(1, 9, 6)),
        tables(gk, edges))
    # a detection's own area on the edges too: a 32 x 32 and a 96 x 96 spread, unmatched
    d32, d96 = person(rng, 900, 900, 10.0), person(rng, 1200, 900, 10.0)
    d32[0, :2], d32[1, :2] = (884.0, 884.0), (916.0, 916.0)
    d96[0, :2], d96[1, :2] = (1152.0, 852.0), (1248.0, 948.0)
    add("detection_areas_on_the_range_edges", (np.array([d32, d96]), [2.0, 1.0]), tables([person(rng, 100, 100, 50.0, 12)], [1500.0]))
    g_small = person(rng, 100, 100, 12.0, 17)
    add("e_above_708", (np.array([detect(rng, g_small, 12.0, 0.05), detect(rng, g_small, 12.0, 0.05) + [1e4, 0, 0],
                                  detect(rng, g_small, 12.0, 0.05) + [30.0, 20.0, 0]]), [3.0, 2.0, 1.0]),
        tables([g_small], [100.0]))
    dets, gts = scene(rng, 3, 4, visible=13)
    add("negative_coordinates", (dets[0] - [700.0, 500.0, 0.0], dets[1]), (gts[0] - [700.0, 500.0, 0.0],) + (gts[1], gts[2] - [700.0, 500.0, 0, 0]) + gts[3:])
    dets, gts = scene(rng, 3, 4, visible=17)
    add("coordinates_of_1e6", (dets[0] + [1e6, 1e6, 0.0], dets[1]), (gts[0] + [1e6, 1e6, 0.0],) + (gts[1], gts[2] + [1e6, 1e6, 0, 0]) + gts[3:])
    dets, gts = scene(rng, 3, 5, visible=15)
    add("nan_score", (dets[0], [2.0, np.nan, 7.0, -np.inf, 1.0]), gts)
    # ---- seeded scenes ----
    while len(out) < 48:
        G, D = int(rng.integers(1, 7)), int(rng.integers(1, 9))
        dets, gts = scene(rng, G, D)
        kp, area, bbox, ignore, crowd = gts
        crowd = (rng.uniform(size=G) < 0.15).astype(np.uint8)
        add("scene_%d" % len(out), dets, tables(kp, area, bbox, crowd=crowd))
    return out


_CACHE = {}


def all_frames():
    if "frames" not in _CACHE:
        _CACHE["frames"] = frames()
    return _CACHE["frames"]


def references(K):
    """match_np of every frame (K = the keypoint_eval module), computed once."""
    if "ref" not in _CACHE:
        _CACHE["ref"] = [K.match_np(d[0], d[1], *g, max_dets=MAX_DETS) for _, d, g in all_frames()]
    return _CACHE["ref"]
