"""Haar cascade face finding: ``cv2.CascadeClassifier(...).detectMultiScale`` of the reference's
camera_face_demo.py, stated in NumPy and run on the device (csrc/haar.hip).

The NumPy functions here (``load_cascade``, ``scales``, ``grey_np``, ``resize_np``, ``integrals_np``,
``result_map_np``, ``candidates_np``, ``group_rectangles_np``, ``detect_np``) are the contract: they
restate OpenCV's CascadeClassifierImpl for new-format stump cascades one rounded operation at a time,
and the kernels equal them bit for bit.  Parity with any OpenCV build is NOT pinned: there is no
OpenCV to compare with where this project is built and tested, so only the call and its arguments
(scaleFactor=1.2, minNeighbors=3, minSize=(1, 1)) are pinned to the reference.

``CascadeClassifier`` is the device path behind the reference's line
``cascade.detectMultiScale(gray_img, scaleFactor=1.2, minNeighbors=3, minSize=(1, 1))``.
"""
import gzip
import os
import xml.etree.ElementTree as ET

import numpy as np

MAX_WINDOW = 64       # largest window side the loader and the kernels take
MAX_SCALES = 64       # most pyramid layers of one frame
MAX_SIDE = 16384      # largest frame side
MAX_CANDIDATES = 4096  # default per-frame cap of the device's candidate list
DEFAULTS = dict(scale_factor=1.2, min_neighbors=3, min_size=(1, 1), max_size=None)  # the reference's call
_KEYS = ("win", "stage_first", "stage_thr", "rects", "weights", "thr", "left", "right")


# ---------------------------------------------------------------- loader
def _check_cascade(c):
    win_w, win_h = int(c["win"][0]), int(c["win"][1])
    if not (3 <= win_w <= MAX_WINDOW and 3 <= win_h <= MAX_WINDOW):
        raise ValueError("window %d x %d: larger than %d x %d (or below 3 x 3)" % (win_w, win_h, MAX_WINDOW, MAX_WINDOW))
    r, w = c["rects"], c["weights"]
    used = np.ones(w.shape, bool)
    used[:, 2] = w[:, 2] != 0
    x, y, rw, rh = r[..., 0], r[..., 1], r[..., 2], r[..., 3]
    bad = used & ((x < 0) | (y < 0) | (rw < 0) | (rh < 0) | (x + rw > win_w) | (y + rh > win_h))
    if bad.any():
        j, k = np.argwhere(bad)[0]
        raise ValueError("stump %d: rect %s lies outside the %d x %d window" % (j, tuple(int(v) for v in r[j, k]), win_w, win_h))
    return c


def load_cascade(path):
    """An ``opencv-cascade-classifier`` XML, plain or gzip-compressed (``.gz``), with stageType BOOST,
    featureType HAAR, stumps only and upright features of 2 or 3 rects, or the compact ``.npz`` ``save_cascade`` writes -> dict of arrays:
    ``win`` (w, h) int32, ``stage_first`` (n_stages + 1,) int32, ``stage_thr`` (n_stages,) f32
    (= float32(stageThreshold) - float32(1e-5)), and per stump in file order ``rects`` (n, 3, 4) int32
    as x, y, w, h, ``weights`` (n, 3) f32 (0 for a missing third rect), ``thr``, ``left``, ``right`` f32.
    ValueError, naming what was found, for anything else."""
    if str(path).endswith(".npz"):
        with np.load(path) as z:
            return _check_cascade({k: z[k] for k in _KEYS})
    if str(path).endswith(".gz"):  # the XML, gzip-compressed (the fixture of the tests)
        with gzip.open(path, "rb") as f:
            root = ET.parse(f).getroot()
    else:
        root = ET.parse(path).getroot()
    node = None
    for child in root:
        tid = child.get("type_id")
        if tid == "opencv-haar-classifier":
            raise ValueError("old-format cascade <%s type_id=%r>: convert it to the opencv-cascade-classifier format"
                             % (child.tag, tid))
        if tid == "opencv-cascade-classifier":
            node = child
    if node is None:
        raise ValueError("no <cascade type_id=\"opencv-cascade-classifier\"> in %s (found %s)"
                         % (os.path.basename(str(path)), [c.tag for c in root]))
    stage_type = (node.findtext("stageType") or "").strip()
    feature_type = (node.findtext("featureType") or "").strip()
    if stage_type != "BOOST":
        raise ValueError("stageType %r: only BOOST is supported" % stage_type)
    if feature_type != "HAAR":
        raise ValueError("featureType %r: only HAAR is supported (LBP and HOG are not)" % feature_type)
    win = np.array([int(node.findtext("width")), int(node.findtext("height"))], np.int32)
    feats = []
    for i, f in enumerate(node.find("features")):
        tilted = (f.findtext("tilted") or "0").strip()
        if tilted not in ("0", ""):
            raise ValueError("feature %d is tilted (<tilted>%s</tilted>): only upright features are supported" % (i, tilted))
        rects = [r.text.split() for r in f.find("rects")]
        if not 2 <= len(rects) <= 3 or any(len(r) != 5 for r in rects):
            raise ValueError("feature %d has %d rects: 2 or 3 of x y w h weight are supported" % (i, len(rects)))
        feats.append(rects)
    first, sthr, rr, ww, thr, left, right = [0], [], [], [], [], [], []
    for s, stage in enumerate(node.find("stages")):
        sthr.append(np.float32(float(stage.findtext("stageThreshold"))) - np.float32(1e-5))
        for weak in stage.find("weakClassifiers"):
            nodes = weak.findtext("internalNodes").split()
            leaves = weak.findtext("leafValues").split()
            if len(nodes) != 4 or len(leaves) != 2 or int(nodes[0]) != 0 or int(nodes[1]) != -1:
                raise ValueError("stage %d: a tree with internalNodes %r (%d leaves): only stumps (0 -1 <feature> "
                                 "<threshold>, 2 leaves) are supported" % (s, " ".join(nodes), len(leaves)))
            fi = int(nodes[2])
            if not 0 <= fi < len(feats):
                raise ValueError("stage %d: feature index %d outside the %d features" % (s, fi, len(feats)))
            r3 = np.zeros((3, 4), np.int32)
            w3 = np.zeros(3, np.float32)
            for k, r in enumerate(feats[fi]):
                r3[k] = [int(v) for v in r[:4]]
                w3[k] = np.float32(float(r[4]))
            rr.append(r3)
            ww.append(w3)
            thr.append(np.float32(float(nodes[3])))
            left.append(np.float32(float(leaves[0])))
            right.append(np.float32(float(leaves[1])))
        first.append(len(thr))
    if not sthr or first[-1] == 0 or any(b <= a for a, b in zip(first, first[1:])):
        raise ValueError("a cascade needs at least one stage and every stage at least one stump (found stages of %s)"
                         % np.diff(first).tolist())
    return _check_cascade({
        "win": win, "stage_first": np.asarray(first, np.int32), "stage_thr": np.asarray(sthr, np.float32),
        "rects": np.asarray(rr, np.int32).reshape(-1, 3, 4), "weights": np.asarray(ww, np.float32).reshape(-1, 3),
        "thr": np.asarray(thr, np.float32), "left": np.asarray(left, np.float32), "right": np.asarray(right, np.float32)})


def save_cascade(path, cascade):
    """The compact form ``load_cascade`` reads back exactly (path ends in .npz)."""
    np.savez_compressed(path, **{k: cascade[k] for k in _KEYS})


# ---------------------------------------------------------------- pyramid
def _rint(v):
    return int(np.rint(v))  # half to even


def scales(h, w, win, scale_factor=1.2, min_size=(1, 1), max_size=None):
    """-> [(float32 factor, layer_w, layer_h)]: the factor starts at 1 (double) and is multiplied by
    scale_factor; the scaled window (rint(win_w f), rint(win_h f)) ends the list once it exceeds max_size
    (default: the image) or the image, and the scale is skipped while it is below min_size."""
    scale_factor = float(scale_factor)
    if not np.isfinite(scale_factor) or scale_factor < 1.01:
        raise ValueError("scale_factor %r: must be finite and >= 1.01" % scale_factor)
    if min(min_size) < 1 or (max_size is not None and min(max_size) < 1):
        raise ValueError("min_size / max_size must be positive")
    win_w, win_h = int(win[0]), int(win[1])
    max_w, max_h = (w, h) if max_size is None else (int(max_size[0]), int(max_size[1]))
    out, factor = [], 1.0
    while True:
        ww, wh = _rint(win_w * factor), _rint(win_h * factor)
        if ww > max_w or wh > max_h or ww > w or wh > h:
            break
        if not (ww < int(min_size[0]) or wh < int(min_size[1])):
            sc = np.float32(factor)
            out.append((sc, _rint(w / float(sc)), _rint(h / float(sc))))
            if len(out) > MAX_SCALES:
                raise ValueError("more than %d scales" % MAX_SCALES)
        factor *= scale_factor
    return out


def grey_np(img):
    """(h, w, 3) BGR u8 -> (1868 B + 9617 G + 4899 R + 8192) >> 14; a 2-D u8 image is grey already."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] != 3):
        raise ValueError("an image is (h, w) or (h, w, 3) uint8, not %s %s" % (img.dtype, img.shape))
    if img.ndim == 2:
        return np.ascontiguousarray(img)
    v = img.astype(np.int32)
    return ((1868 * v[..., 0] + 9617 * v[..., 1] + 4899 * v[..., 2] + 8192) >> 14).astype(np.uint8)


def _axis(dst, src):
    f = (np.arange(dst, dtype=np.float64) + 0.5) * (float(src) / float(dst)) - 0.5
    cell = np.floor(f)
    a = np.rint((f - cell) * 256.0).astype(np.int64)
    cell = cell.astype(np.int64)
    return np.clip(cell, 0, src - 1), np.clip(cell + 1, 0, src - 1), a


def resize_np(grey, lw, lh):
    """Integer bilinear, pixel centres aligned: f = (d + 0.5) src/dst - 0.5, upper weight
    rint(frac 256), indices clamped; the horizontal pass gives 8.8 values (uint16), the vertical pass
    (acc + 32768) >> 16."""
    h, w = grey.shape
    x0, x1, ax = _axis(lw, w)
    y0, y1, ay = _axis(lh, h)
    g = grey.astype(np.int64)
    hor = (g[:, x0] * (256 - ax) + g[:, x1] * ax).astype(np.uint16).astype(np.int64)
    acc = hor[y0] * (256 - ay)[:, None] + hor[y1] * ay[:, None]
    return ((acc + 32768) >> 16).astype(np.uint8)


def integrals_np(layer):
    """-> (sum int32, sqsum uint32 modulo 2^32), each with an extra zero row and column."""
    h, w = layer.shape
    v = layer.astype(np.uint64)
    s = np.zeros((h + 1, w + 1), np.uint64)
    q = np.zeros((h + 1, w + 1), np.uint64)
    s[1:, 1:] = v.cumsum(0).cumsum(1)
    q[1:, 1:] = (v * v).cumsum(0).cumsum(1)
    return (s & 0xFFFFFFFF).astype(np.uint32).view(np.int32), (q & 0xFFFFFFFF).astype(np.uint32)


def pyramid_np(img, cascade, scale_factor=1.2, min_size=(1, 1), max_size=None):
    """-> [dict(scale f32, pixels, sum, sqsum, step, ys, xs)] per layer (ys, xs: the step grid)."""
    g = grey_np(img)
    h, w = g.shape
    win_w, win_h = int(cascade["win"][0]), int(cascade["win"][1])
    out = []
    for sc, lw, lh in scales(h, w, cascade["win"], scale_factor, min_size, max_size):
        pix = resize_np(g, lw, lh)
        s, q = integrals_np(pix)
        step = 1 if float(sc) >= 2.0 else 2
        out.append(dict(scale=sc, pixels=pix, sum=s, sqsum=q, step=step,
                        ys=np.arange(0, lh - win_h, step), xs=np.arange(0, lw - win_w, step)))
    return out


# ---------------------------------------------------------------- the classifier
def _rect_sum(a, ys, xs, r):
    x, y, w, h = int(r[0]), int(r[1]), int(r[2]), int(r[3])
    return a[ys + y, xs + x] - a[ys + y, xs + x + w] - a[ys + y + h, xs + x] + a[ys + y + h, xs + x + w]


def _windows(cascade, layer, ys, xs):
    """setWindow at the positions (ys, xs): -> (valid, vnf f32)."""
    win_w, win_h = int(cascade["win"][0]), int(cascade["win"][1])
    norm = (1, 1, win_w - 2, win_h - 2)
    area = (win_w - 2) * (win_h - 2)
    with np.errstate(over="ignore"):
        vs = _rect_sum(layer["sum"], ys, xs, norm).astype(np.float64)
        vq = _rect_sum(layer["sqsum"], ys, xs, norm).astype(np.float64)
    nf = float(area) * vq - vs * vs
    pos = nf > 0
    vnf = np.ones(nf.shape, np.float32)
    vnf[pos] = (1.0 / np.sqrt(nf[pos])).astype(np.float32)
    valid = pos & (np.float32(area) * vnf < np.float32(0.1))
    return valid, vnf


def _stage(cascade, k, layer, ys, xs, vnf):
    """Stage k at the positions: -> passed (bool)."""
    first = cascade["stage_first"]
    total = np.zeros(len(ys), np.float32)
    with np.errstate(over="ignore"):
        for j in range(int(first[k]), int(first[k + 1])):
            r, wt = cascade["rects"][j], cascade["weights"][j]
            v = wt[0] * _rect_sum(layer["sum"], ys, xs, r[0]).astype(np.float32) \
                + wt[1] * _rect_sum(layer["sum"], ys, xs, r[1]).astype(np.float32)
            if wt[2] != 0:
                v = v + wt[2] * _rect_sum(layer["sum"], ys, xs, r[2]).astype(np.float32)
            v = v * vnf
            total = total + np.where(v < cascade["thr"][j], cascade["left"][j], cascade["right"][j])
    return ~(total < cascade["stage_thr"][k])


def _layer_map(cascade, layer):
    n_stages = len(cascade["stage_thr"])
    ys, xs = layer["ys"], layer["xs"]
    m = np.full((len(ys), len(xs)), -2, np.int8)
    if m.size == 0:
        return m
    gy, gx = np.meshgrid(ys, xs, indexing="ij")
    valid, vnf = _windows(cascade, layer, gy.ravel(), gx.ravel())
    pass0 = _stage(cascade, 0, layer, gy.ravel(), gx.ravel(), vnf).reshape(m.shape)
    valid = valid.reshape(m.shape)
    skip = valid & ~pass0  # a visited window of this kind hides its right neighbour
    visited = np.ones(m.shape, bool)
    for i in range(1, m.shape[1]):
        visited[:, i] = ~(visited[:, i - 1] & skip[:, i - 1])
    m[visited & ~valid] = -1
    m[visited & valid & ~pass0] = 0
    live = visited & valid & pass0
    iy, ix = np.nonzero(live)
    vnf = vnf.reshape(m.shape)[iy, ix]
    for k in range(1, n_stages):
        if not len(iy):
            break
        ok = _stage(cascade, k, layer, ys[iy], xs[ix], vnf)
        m[iy[~ok], ix[~ok]] = k
        iy, ix, vnf = iy[ok], ix[ok], vnf[ok]
    m[iy, ix] = n_stages
    return m


def result_map_np(img, cascade, scale_factor=1.2, min_size=(1, 1), max_size=None):
    """Per layer an int8 map over the step grid: n_stages passed, k failed stage k, -1 invalid window
    (setWindow refused it), -2 never looked at (its left neighbour was valid and failed stage 0:
    OpenCV's ``if (result == 0) x += yStep``).  -> (maps, layers)."""
    layers = pyramid_np(img, cascade, scale_factor, min_size, max_size)
    return [_layer_map(cascade, l) for l in layers], layers


def _candidate_rects(cascade, maps, layers):
    n_stages = len(cascade["stage_thr"])
    win_w, win_h = int(cascade["win"][0]), int(cascade["win"][1])
    out = []
    for m, l in zip(maps, layers):
        sc = float(l["scale"])
        iy, ix = np.nonzero(m == n_stages)  # row-major: (y, x) order
        for y, x in zip(l["ys"][iy], l["xs"][ix]):
            out.append((_rint(x * sc), _rint(y * sc), _rint(win_w * sc), _rint(win_h * sc)))
    return np.asarray(out, np.int32).reshape(-1, 4)


def candidates_np(img, cascade, scale_factor=1.2, min_size=(1, 1), max_size=None):
    """The windows that pass every stage, as (x, y, w, h) int32 in (layer, y, x) order."""
    maps, layers = result_map_np(img, cascade, scale_factor, min_size, max_size)
    return _candidate_rects(cascade, maps, layers)


def similar_rects(a, b, eps=0.2):
    delta = eps * (min(int(a[2]), int(b[2])) + min(int(a[3]), int(b[3]))) * 0.5
    return (abs(int(a[0]) - int(b[0])) <= delta and abs(int(a[1]) - int(b[1])) <= delta
            and abs(int(a[0]) + int(a[2]) - int(b[0]) - int(b[2])) <= delta
            and abs(int(a[1]) + int(a[3]) - int(b[1]) - int(b[3])) <= delta)


def group_rectangles_np(rects, min_neighbors, eps=0.2):
    """cv::groupRectangles: -> (rects (n, 4) int32, neighbours (n,) int32)."""
    rects = np.asarray(rects, np.int32).reshape(-1, 4)
    n = len(rects)
    if min_neighbors <= 0 or n == 0:
        return rects.copy(), np.ones(n, np.int32)
    parent = list(range(n))

    def root(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for i in range(n):
        for j in range(i + 1, n):
            if similar_rects(rects[i], rects[j], eps):
                a, b = root(i), root(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    label, classes = {}, []
    for i in range(n):  # classes numbered by their first member
        r = root(i)
        if r not in label:
            label[r] = len(classes)
            classes.append([])
        classes[label[r]].append(i)
    mean, count = [], []
    for members in classes:
        s = rects[members].astype(np.int64).sum(0)
        inv = np.float32(1.0) / np.float32(len(members))
        mean.append([_rint(np.float32(v) * inv) for v in s])
        count.append(len(members))
    out_r, out_n = [], []
    for i, (r1, n1) in enumerate(zip(mean, count)):
        if n1 <= min_neighbors:
            continue
        for j, (r2, n2) in enumerate(zip(mean, count)):
            if j == i or n2 <= min_neighbors:
                continue
            dx, dy = int(r2[2] * eps), int(r2[3] * eps)
            if (r1[0] >= r2[0] - dx and r1[1] >= r2[1] - dy and r1[0] + r1[2] <= r2[0] + r2[2] + dx
                    and r1[1] + r1[3] <= r2[1] + r2[3] + dy and (n2 > max(3, n1) or n1 < 3)):
                break
        else:
            out_r.append(r1)
            out_n.append(n1)
    return np.asarray(out_r, np.int32).reshape(-1, 4), np.asarray(out_n, np.int32)


def detect_np(img, cascade, scale_factor=1.2, min_neighbors=3, min_size=(1, 1), max_size=None):
    """-> (rects (n, 4) int32 as x, y, w, h, neighbours (n,) int32)."""
    return group_rectangles_np(candidates_np(img, cascade, scale_factor, min_size, max_size), min_neighbors, 0.2)


# ---------------------------------------------------------------- the device path
class CascadeClassifier(object):
    """``cv2.CascadeClassifier`` for this project: the cascade is uploaded once to ``device``; every
    call runs grey, pyramid, integrals and the cascade on the device and groups on the host in C++."""

    def __init__(self, path, device=0):
        from . import _lib
        self._lib = _lib
        self.cascade = load_cascade(path)
        self.device = int(device)
        self._h = _lib.HaarHandle(self.cascade, self.device)

    def close(self):
        if self._h is not None:
            self._h.close()
            self._h = None

    def empty(self):
        return self._h is None

    def detect_batch(self, frames, scaleFactor=1.2, minNeighbors=3, minSize=(1, 1), maxSize=None,
                     max_candidates=MAX_CANDIDATES, with_neighbours=False):
        """frames: (h, w, 3) BGR or (h, w) grey uint8 arrays of any mix of sizes -> a list of (n, 4)
        int32 arrays (x, y, w, h); with_neighbours: (rects, neighbours) pairs."""
        # a frame has no more rectangles than candidates: max_candidates rows always hold them
        rects, neigh, count, status = self._h.detect(frames, scaleFactor, minNeighbors, minSize, maxSize,
                                                     max_candidates, int(max_candidates))
        if (status != 0).any():
            raise RuntimeError("a frame has %d candidates: raise max_candidates (%d)" % (count.max(), max_candidates))
        out =[(rects[f, :count[f]].copy(), neigh[f, :count[f]].copy()) for f in range(len(frames))]
        return out if with_neighbours else [r for r, _ in out]

    def detectMultiScale(self, img, scaleFactor=1.2, minNeighbors=3, minSize=(1, 1), maxSize=None):
        """-> (n, 4) int32 (x, y, w, h): the reference's call with only the import changed."""
        return self.detect_batch([img], scaleFactor, minNeighbors, minSize, maxSize)[0]

    def detect_staged(self, pose_ctx, first, n, scaleFactor=1.2, minNeighbors=3, minSize=(1, 1), maxSize=None,
                      max_candidates=MAX_CANDIDATES, with_neighbours=False):
        """The same on frames [first, first + n) of ``pose_ctx``'s staged set (a ``_lib.Context`` or a
        PoseDetector), read in place after the context's queued work: only tables go up, only
        rectangles come back."""
        ctx = getattr(pose_ctx, "ctx", pose_ctx)
        cap = int(max_candidates)
        rects, neigh, count, status = self._h.detect_staged(ctx, first, n, scaleFactor, minNeighbors, minSize, maxSize,
                                                            max_candidates, cap)
        if (status != 0).any():
            raise RuntimeError("a staged frame has %d candidates: raise max_candidates (%d)" % (count.max(), max_candidates))
        out = [(rects[f, :count[f]].copy(), neigh[f, :count[f]].copy()) for f in range(n)]
        return out if with_neighbours else [r for r, _ in out]
