"""The ``--vis`` viewer of gen_ignore_mask.py: annotation masks tinted onto the frame with the
keypoints marked (draw_masks_and_keypoints, :48-71) beside the mask_miss tint (dwaw_gen_masks, :39-46).

The ``*_np`` functions are the statement: plain NumPy that defines every byte, pinned to the
reference's own two functions by tests/golden/maskview/*.npz.  The picture is not a blend of two
uint8 images: the first tint turns the frame into a float64 image that is carried from annotation
to annotation, ``cv2.circle`` paints 255.0 / 0.0 onto that float image between tints, the next tint
runs over those discs, and the one cast to uint8 comes at the end.  So it depends on the order of the
annotations and on the unrounded state.

``cv2.circle`` is not installed here; the disc is ``draw.draw_disc`` (the pixels within radius 3),
through a ``draw.Raster``, so edge pixels can differ from OpenCV's: rendering parity stays unpinned,
exactly as for ``draw_person_pose``.  The per-annotation masks are ``masks.ann_to_mask_np``
(pycocotools' rasteriser restated, unpinned likewise).

``views`` / ``panels`` run on the device (op_annotation_views, csrc/maskview.hip) and equal ``view_np``
/ ``panel_np`` byte for byte; they raise when the library or the device is missing (there is no CPU
path).  No window is opened: there is no cv2 here, the panels are returned or written as PNGs
(``python -m ....gen_ignore_mask --vis``).

Declared limits (ValueError naming the annotation's id): ``keypoints`` whose length is not a multiple
of 3; a keypoint coordinate that is not an integer or exceeds 32768 in magnitude (the reference hands
them to ``cv2.circle``, which takes integers); the segmentation limits of
``masks.segmentation_parts``; and a frame that is not (h, w, 3) uint8.
"""
import ctypes

import numpy as np

from . import _lib
from . import draw as _draw
from . import masks as _masks

ALPHA = 0.7
RADIUS = 3
MAX_COORD = 32768
COLOR_CROWD, COLOR_NO_KEYPOINTS, COLOR_PERSON = (0, 0, 1), (0, 1, 0), (1, 0, 0)
DISC_COLORS = {1: (255, 255, 0), 2: (255, 0, 255)}
# op_annotation_views' tint codes: the BGR channel a colour raises
TINT_CODE = {COLOR_PERSON: 0, COLOR_NO_KEYPOINTS: 1, COLOR_CROWD: 2}


# ---- the statement ----
def _frame(img, who):
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("%s: an (h, w, 3) uint8 frame expected" % who)
    return img


def tint_np(img, mask, color):
    """One step of the reference (:58-63, :40-45): float64 ``(img + 0.7 * clmsk) - 0.7 * mskd`` over all
    pixels, ``clmsk = ones * mask3 * color * 255`` and ``mskd = img * mask3``; ``img`` is the uint8
    frame on the first step and the float64 result afterwards."""
    bimsk = np.repeat(np.asarray(mask)[:, :, np.newaxis], 3, axis=2)
    mskd = img * bimsk.astype(np.int32)
    clmsk = np.ones(bimsk.shape) * bimsk
    for i in range(3):
        clmsk[:, :, i] = clmsk[:, :, i] * color[i] * 255
    return img + ALPHA * clmsk - ALPHA * mskd


def ann_color(ann):
    """The tint of an annotation's mask (:52-57)."""
    if ann["iscrowd"] == 1:
        return COLOR_CROWD
    if ann["num_keypoints"] == 0:
        return COLOR_NO_KEYPOINTS
    return COLOR_PERSON


def keypoint_triples(ann):
    """``np.array(ann['keypoints']).reshape(-1, 3)`` (:66) as int32 (k, 3), checked against the
    declared limits."""
    def bad(why):
        return ValueError("annotation %r: %s" % (ann.get("id"), why))

    kp = np.asarray(ann.get("keypoints", []))
    if kp.ndim != 1 or kp.size % 3:
        raise bad("keypoints: %s numbers (a flat list of x, y, v triples)" % (kp.shape,))
    if kp.size == 0:
        return np.zeros((0, 3), np.int32)
    if kp.dtype.kind not in "iuf":
        raise bad("keypoints must be numbers")
    kp = kp.reshape(-1, 3)
    xy = kp[:, :2].astype(np.float64)
    if not np.all(np.isfinite(xy)) or np.any(xy != np.floor(xy)) or np.abs(xy).max() > MAX_COORD:
        raise bad("a keypoint coordinate is not an integer or exceeds %d in magnitude" % MAX_COORD)
    v = kp[:, 2]
    out = np.empty(kp.shape, np.int32)
    out[:, :2] = xy
    out[:, 2] = np.where(v == 1, 1, np.where(v == 2, 2, 0))  # only v == 1 and v == 2 are looked at
    return out


def draw_masks_and_keypoints_np(img, annotations, masks=None, raster=None):
    """draw_masks_and_keypoints (:48-71).  ``masks`` supplies the per-annotation masks instead of
    ``masks.ann_to_mask_np``; ``raster`` is the cv2 stand-in, default ``draw.Raster()``."""
    img = _frame(img, "draw_masks_and_keypoints_np")
    h, w = img.shape[:2]
    cv = raster if raster is not None else _draw.Raster()
    triples = [keypoint_triples(ann) for ann in annotations]
    for k, ann in enumerate(annotations):
        mask = (np.asarray(masks[k]) if masks is not None else _masks.ann_to_mask_np(ann, h, w)).astype(np.uint8)
        img = tint_np(img, mask, ann_color(ann))
        for x, y, v in triples[k]:
            if v in DISC_COLORS:
                cv.circle(img, (int(x), int(y)), RADIUS, DISC_COLORS[int(v)], -1)
    return img.astype(np.uint8)


def draw_gen_masks_np(img, mask, color=(0, 0, 1)):
    """dwaw_gen_masks (:39-46): one tint of the uint8 frame, cast."""
    img = _frame(img, "draw_gen_masks_np")
    return tint_np(img, np.asarray(mask), color).astype(np.uint8)


def view_np(img, annotations):
    """What ``--vis`` shows for one image: (ann_img, msk_img), the annotation view and the tint of
    ``gen_masks``' mask_miss."""
    img = _frame(img, "view_np")
    h, w = img.shape[:2]
    per = [_masks.ann_to_mask_np(ann, h, w) for ann in annotations]
    ann_img = draw_masks_and_keypoints_np(img, annotations, masks=per)
    msk_img = draw_gen_masks_np(img, _masks.gen_masks_np(annotations, h, w, masks=per)[1])
    return ann_img, msk_img


def panel_np(img, annotations):
    """``np.hstack((ann_img, msk_img))`` (:106): (h, 2 w, 3) uint8."""
    return np.hstack(view_np(img, annotations))


# ---- the device ----
def pack_views(samples):
    """samples = n of (img, annotations) -> (frames kept alive, the flat arrays of
    op_annotation_views as a dict keyed by its argument names)."""
    frames = [_lib._row_strided_u8(_frame(img, "maskview.views")) for img, _ in samples]
    lists = [list(anns) for _, anns in samples]
    packed = _lib.pack_annotations([(a.shape[0], a.shape[1], anns) for a, anns in zip(frames, lists)])
    triples = [keypoint_triples(ann) for anns in lists for ann in anns]
    kp_offsets = np.zeros(len(triples) + 1, np.int32)
    kp_offsets[1:] = np.cumsum([len(t) for t in triples])
    packed["kp_offsets"] = kp_offsets
    packed["kp"] = np.ascontiguousarray(np.concatenate(triples), np.int32) if triples else np.zeros((0, 3), np.int32)
    packed["ann_tint"] = np.array([TINT_CODE[ann_color(ann)] for anns in lists for ann in anns], np.int32)
    packed["row_stride"] = np.array([a.strides[0] for a in frames], np.int64)
    return frames, packed


def views(samples, device=0, want_ann=True, want_miss=True):
    """``view_np`` of every sample on the device: samples = [(img, annotations), ...] of any sizes ->
    [(ann_img, msk_img), ...] from one call (op_annotation_views).  ``want_ann`` / ``want_miss``: leave
    one of the two out (its entry is None)."""
    frames, packed = pack_views(list(samples))
    shapes = [(a.shape[0], a.shape[1], 3) for a in frames]
    out_ann = [np.empty(s, np.uint8) for s in shapes] if want_ann else None
    out_miss = [np.empty(s, np.uint8) for s in shapes] if want_miss else None
    _lib.annotation_views_call(int(device), frames, packed, out_ann, out_miss)
    return [(out_ann[f] if want_ann else None, out_miss[f] if want_miss else None) for f in range(len(frames))]


def panels(samples, device=0):
    """``panel_np`` of every sample on the device, one call for the batch."""
    return [np.hstack(pair) for pair in views(samples, device)]


def last_ms(device=0):
    """Device time (ms) of the uploads and kernels of the last ``op_annotation_views`` on ``device``."""
    ms = ctypes.c_double()
    _lib.check(_lib.lib().op_annotation_views_last_ms(int(device), ctypes.byref(ms)), "op_annotation_views_last_ms")
    return ms.value
