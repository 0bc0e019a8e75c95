"""Ignore masks from COCO segmentations (gen_ignore_mask.py:23-37, COCO.annToMask).

The ``*_np`` functions are the statement: plain NumPy / Python that defines every bit of the result.
``poly_toggles`` is pycocotools' ``rleFrPoly`` (maskApi.c) written from memory of its source;
pycocotools is not installed where this was written, so parity with it is unpinned.
``gen_masks_np`` is the reference's ``gen_masks``, pinned to it by tests/golden/masks/gen_*.npz.

``ann_to_mask`` / ``ignore_masks`` run on the device (op_ignore_masks, csrc/masks.hip) and equal the
statement bit for bit; they raise when the library or the device is missing (there is no CPU path,
DESIGN §1).

A segmentation is a list of polygons (``[x0, y0, x1, y1, ...]`` each, the union is taken) or an
uncompressed RLE ``{'size': [h, w], 'counts': [c0, c1, ...]}``.  Both become *toggle positions*: indices
in [0, h * w] of the column-major linear pixel index x * h + y; pixel i is set iff the number of
toggles <= i is odd (over the whole linear index, not per column; equal positions cancel in pairs).

Declared limits (ValueError naming the annotation's id): compressed (string) ``counts``; a polygon
of odd length or of fewer than 3 points (pycocotools reads a list of 4 numbers as a box: not
reproduced); a coordinate that is not finite or exceeds 65536 in magnitude.
"""
import numpy as np

from . import _lib
from .labels import train_params

UPSAMPLE = 5        # rleFrPoly's scale
MAX_COORD = 65536.0
ROLE_KEEP, ROLE_MISS, ROLE_CROWD = 0, 1, 2
KIND_POLYGON, KIND_RLE = 0, 1


# ---- the statement ----
def poly_toggles(xy, h, w):
    """One polygon ``xy[2k]`` (k >= 3 points, float64) -> int64 array of toggle positions."""
    xy = np.asarray(xy, np.float64).ravel()
    k = len(xy) // 2
    if len(xy) % 2 or k < 3:
        raise ValueError("a polygon is an even number of coordinates, at least 3 points; got %d numbers" % len(xy))
    X = [int(UPSAMPLE * float(v) + 0.5) for v in xy[0::2]]  # C's (int): truncation toward zero
    Y = [int(UPSAMPLE * float(v) + 0.5) for v in xy[1::2]]
    X.append(X[0])
    Y.append(Y[0])
    out = []
    for j in range(k):
        xs, ys, xe, ye = X[j], Y[j], X[j + 1], Y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, ys, xe, ye = xe, ye, xs, ys
        if dx == 0 and dy == 0:
            continue  # the single point (xs, ys): nothing to cross
        if dx >= dy:
            s = (ye - ys) / dx
            d = np.arange(dx + 1, dtype=np.int64)
            t = dx - d if flip else d
            u = xs + t
            v = (ys + s * t + 0.5).astype(np.int64)  # three float64 roundings, truncated toward zero
        else:
            s = (xe - xs) / dy
            d = np.arange(dy + 1, dtype=np.int64)
            t = dy - d if flip else d
            v = ys + t
            u = (xs + s * t + 0.5).astype(np.int64)
        i = np.nonzero(u[1:] != u[:-1])[0] + 1
        xd = np.where(u[i] < u[i - 1], u[i], u[i] - 1).astype(np.float64)
        xd = (xd + 0.5) / UPSAMPLE - 0.5
        ok = (np.floor(xd) == xd) & (xd >= 0) & (xd <= w - 1)
        yd = np.minimum(v[i], v[i - 1]).astype(np.float64)
        yd = np.ceil(np.clip((yd + 0.5) / UPSAMPLE - 0.5, 0, h))
        out.append((xd[ok] * h + yd[ok]).astype(np.int64))
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def rle_toggles(counts, h, w, size=None):
    """An uncompressed RLE (runs of 0s and 1s alternating, column-major, 0s first) -> its toggles:
    the running sums of the counts, the last one h * w."""
    if size is not None and [int(v) for v in size] != [h, w]:
        raise ValueError("RLE size %r, the image is %r" % (list(size), [h, w]))
    c = np.asarray(counts)
    if c.ndim != 1 or (len(c) and (c.dtype.kind not in "iu" or c.min() < 0)):
        raise ValueError("RLE counts must be a list of non-negative integers")
    c = c.astype(np.int64)
    if int(c.sum()) != h * w:
        raise ValueError("RLE counts sum to %d, the image has %d pixels" % (int(c.sum()), h * w))
    return np.cumsum(c)


def toggles_to_mask(toggles, h, w):
    """Step 4: (h, w) bool, flat column-major pixel i set iff the number of toggles <= i is odd."""
    flips = np.bincount(np.asarray(toggles, np.int64), minlength=h * w + 1)[:h * w] & 1
    return (np.cumsum(flips) & 1).astype(bool).reshape(w, h).T.copy()


def segmentation_parts(ann, h, w):
    """The parts of an annotation's segmentation, checked against the declared limits:
    [(KIND_POLYGON, float64[2k]) | (KIND_RLE, uint32[m]), ...]."""
    def bad(why):
        return ValueError("annotation %r: %s" % (ann.get("id"), why))

    seg = ann["segmentation"]
    if isinstance(seg, dict):
        counts = seg.get("counts")
        if isinstance(counts, (str, bytes)):
            raise bad("compressed RLE counts are not supported")
        try:
            rle_toggles(counts, h, w, seg.get("size"))
        except ValueError as e:
            raise bad(str(e))
        return [(KIND_RLE, np.asarray(counts, np.uint32))]
    parts = []
    for poly in seg:
        xy = np.asarray(poly, np.float64).ravel()
        if len(xy) % 2 or len(xy) < 6:
            raise bad("a polygon of %d numbers (an even count, at least 3 points)" % len(xy))
        if not np.all(np.isfinite(xy)) or np.abs(xy).max() > MAX_COORD:
            raise bad("a polygon coordinate is not finite or exceeds %d in magnitude" % MAX_COORD)
        parts.append((KIND_POLYGON, xy))
    return parts


def ann_to_mask_np(ann, h, w):
    """COCO.annToMask: the union of the polygons' masks, or the RLE's mask; (h, w) bool."""
    mask = np.zeros((h, w), bool)
    for kind, data in segmentation_parts(ann, h, w):
        mask |= toggles_to_mask(poly_toggles(data, h, w) if kind == KIND_POLYGON else rle_toggles(data, h, w), h, w)
    return mask


def ann_role(ann):
    """What gen_masks does with an annotation's mask (gen_ignore_mask.py:28-36)."""
    if ann["iscrowd"] == 1:
        return ROLE_CROWD
    if ann["num_keypoints"] < train_params["min_keypoints"] or ann["area"] <= train_params["min_area"]:
        return ROLE_MISS
    return ROLE_KEEP


def gen_masks_np(annotations, h, w, masks=None):
    """gen_masks (gen_ignore_mask.py:23-37) over the annotations in order -> (mask_all, mask_miss);
    ``masks`` supplies the per-annotation masks instead of ``ann_to_mask_np``."""
    mask_all, mask_miss = np.zeros((h, w), bool), np.zeros((h, w), bool)
    for k, ann in enumerate(annotations):
        mask = np.asarray(masks[k]).astype(bool) if masks is not None else ann_to_mask_np(ann, h, w)
        role = ann_role(ann)
        if role == ROLE_CROWD:
            mask_miss = mask_miss | (mask & ~mask_all)
        elif role == ROLE_MISS:
            mask_miss = mask_miss | mask
        mask_all = mask_all | mask
    return mask_all, mask_miss


# ---- the device ----
def _run(images, device, want_ann):
    packed = _lib.pack_annotations(images)
    n = len(images)
    all_ = [np.empty((h, w), np.uint8) for h, w, _ in images]
    miss = [np.empty((h, w), np.uint8) for h, w, _ in images]
    per = [np.empty((h, w), np.uint8) for h, w, anns in images for _ in anns] if want_ann else None
    _lib.ignore_masks_call(int(device), n, packed, all_, miss, per)
    return all_, miss, per


def ann_to_mask(ann, h, w, device=0):
    """``ann_to_mask_np`` on the device: (h, w) bool."""
    _, _, per = _run([(int(h), int(w), [ann])], device, True)
    return per[0].astype(bool)


def ignore_masks(images, device=0):
    """images = n of (h, w, annotations) -> n of (mask_all, mask_miss) bool arrays: ``gen_masks_np``
    of every image, one device call for the batch."""
    images = [(int(h), int(w), list(anns)) for h, w, anns in images]
    all_, miss, _ = _run(images, device, False)
    return [(a.astype(bool), m.astype(bool)) for a, m in zip(all_, miss)]


def last_ms(device=0):
    """Device time (ms) of the uploads and kernels of the last ``op_ignore_masks`` on ``device``."""
    import ctypes
    ms = ctypes.c_double()
    _lib.check(_lib.lib().op_ignore_masks_last_ms(int(device), ctypes.byref(ms)), "op_ignore_masks_last_ms")
    return ms.value
