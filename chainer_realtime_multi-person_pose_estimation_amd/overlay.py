"""PAFs, heat maps and the ignore mask over a frame: the viewer of coco_data_loader.py (:29-59,
:372-382), as a NumPy statement and as one kernel launch per batch.

The statement mirrors the reference function by function: ``overlay_paf_np`` / ``overlay_pafs_np``
(hue = direction, saturation = value = magnitude), ``overlay_heatmap_np`` (the JET colour map),
``overlay_ignore_mask_np`` and ``overlay_np``, the ``__main__`` sequence: the maps are resized to the
frame, then PAFs, heat and mask are applied in that order.  Images are uint8 (h, w, 3) BGR, maps
float32 (C, mh, mw).  ``overlay`` / ``overlay_staged`` paint a batch on the device (op_overlay /
op_overlay_staged, csrc/overlay.hip) and agree with ``overlay_np`` bit for bit, given that no pixel's
``hue * 255`` lies on a whole number's edge (``hue_margin``): every step but the float64 ``arctan2`` is
an exactly rounded operation in both worlds.

What the reference computes itself (the HSV image handed to ``cv2.cvtColor``, the index image handed
to ``cv2.applyColorMap``, the masked product) is pinned to its own code by
tests/golden/overlay/*.npz.  Three OpenCV pieces are restated and stay unpinned, as the other OpenCV
restatements of this package do (OpenCV is not available to pin them against): the JET table
(``jet_lut``), the float32 linear resize (``resize_linear_f32_np``) and HSV2BGR
(``augment.hsv2bgr_np``).
"""
import ctypes

import numpy as np

from . import _lib
from .augment import hsv2bgr_np, resize_linear_np

f32 = np.float32
MAX_SIDE = 16384
OP_OVERLAY_PAFS, OP_OVERLAY_HEAT = 1, 2
_tables = {}


def add_weighted(a, wa, b, wb, gamma=0.0):
    """``demo.add_weighted``: the blend of every layer (demo.py pulls in the detectors: imported late)."""
    from .demo import add_weighted as blend
    return blend(a, wa, b, wb, gamma)


def jet_lut():
    """(256, 3) uint8 BGR: the analytic JET, entry i at v = i / 255 in float64: r = clip(1.5 - |4v - 3|,
    0, 1), g = clip(1.5 - |4v - 2|, 0, 1), b = clip(1.5 - |4v - 1|, 0, 1), each rint(255 x) to even.
    It stands in for ``cv2.applyColorMap(..., cv2.COLORMAP_JET)`` and is not pinned against OpenCV's
    own table (OpenCV is not installed here); a caller who has that table passes it as ``lut``."""
    if "jet" not in _tables:
        v = np.arange(256, dtype=np.float64) / 255
        ch = [np.clip(1.5 - np.abs(4 * v - k), 0, 1) for k in (1, 2, 3)]  # b, g, r
        lut = np.rint(255 * np.stack(ch, axis=1)).astype(np.uint8)
        lut.setflags(write=False)
        _tables["jet"] = lut
    return _tables["jet"]


def _lut(lut):
    if lut is None:
        return jet_lut()
    lut = np.ascontiguousarray(lut, np.uint8)
    if lut.shape != (256, 3):
        raise ValueError("overlay: lut (256, 3) uint8 BGR expected, got %s" % (lut.shape,))
    return lut


def _coeffs_f32(dsize, ssize):
    """Taps of one axis, in the shape of ``augment._linear_coeffs``: (s0, s1, 1 - f, f)."""
    scale = 1.0 / (float(dsize) / float(ssize))
    f = ((np.arange(dsize, dtype=np.float64) + 0.5) * scale - 0.5).astype(f32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(f32)
    lo, hi = s < 0, s >= ssize - 1
    f[lo | hi] = 0.0
    s[lo] = 0
    s[hi] = ssize - 1
    return s, np.minimum(s + 1, ssize - 1), f32(1.0) - f, f


def resize_linear_f32_np(x, oh, ow):
    """``cv2.resize(x.transpose(1, 2, 0), (ow, oh)).transpose(2, 0, 1)`` (INTER_LINEAR) on float32 (C,
    mh, mw): per axis f = float32((d + 0.5) * scale - 0.5), s = floor(f), f -= s, clamped to the source
    ((0, 0) below it, (ssize - 1, 0) at its last sample), weights (1 - f, f); the horizontal pass
    first, then the vertical one, every product and sum rounded to float32 on its own.  Equal sizes
    return the input bit for bit.  Not pinned against OpenCV: its float path may contract products."""
    x = np.asarray(x, f32)
    if x.ndim != 3 or min(x.shape[1:]) < 1 or oh < 1 or ow < 1:
        raise ValueError("resize_linear_f32_np: (C, mh, mw) maps and a size >= 1 expected")
    if x.shape[1:] == (oh, ow):
        return x.copy()
    x0, x1, a0, a1 = _coeffs_f32(ow, x.shape[2])
    r0, r1, b0, b1 = _coeffs_f32(oh, x.shape[1])
    hres = x[:, :, x0] * a0 + x[:, :, x1] * a1
    out = hres[:, r0] * b0[:, None] + hres[:, r1] * b1[:, None]
    assert out.dtype == f32
    return out


def paf_hsv_np(paf):
    """The uint8 HSV image ``overlay_paf`` (:30-35) hands to ``cv2.cvtColor``: paf float64 (2, h, w)."""
    paf = np.asarray(paf, np.float64)
    hue = ((np.arctan2(paf[1], paf[0]) / np.pi) / -2 + 0.5)
    saturation = np.sqrt(paf[0] ** 2 + paf[1] ** 2)
    saturation[saturation > 1.0] = 1.0
    value = saturation.copy()
    hsv_paf = np.vstack((hue[np.newaxis], saturation[np.newaxis], value[np.newaxis])).transpose(1, 2, 0)
    return (hsv_paf * 255).astype(np.uint8)


def hue_margin(paf):
    """The smallest distance of ``hue * 255`` (the statement's float64) to a whole number over the
    pixels of paf float64 (2, h, w), hue 0 and hue 255 apart (IEEE ``arctan2`` returns the axes
    exactly).  The device's ``atan2`` may differ from the host's in the last places; a picture whose
    margin exceeds that difference is the same in both."""
    paf = np.asarray(paf, np.float64)
    v = ((np.arctan2(paf[1], paf[0]) / np.pi) / -2 + 0.5) * 255
    d = np.abs(v - np.rint(v))
    d[(v == 0.0) | (v == 255.0)] = 0.5
    return float(d.min())


def overlay_paf_np(img, paf):
    """overlay_paf (:29-37): paf float64 (2, h, w) over img."""
    return add_weighted(img, 0.6, hsv2bgr_np(paf_hsv_np(paf)), 0.4, 0)


def mix_pafs_np(pafs):
    """What overlay_pafs (:39-48) hands to overlay_paf: float64 (2, h, w), the limbs of pafs (2L, h,
    w) added in limb order onto +0.0."""
    pafs = np.asarray(pafs)
    if pafs.ndim != 3 or pafs.shape[0] < 2 or pafs.shape[0] % 2:
        raise ValueError("overlay: pafs (2L, h, w) expected, got %s" % (pafs.shape,))
    mix = np.zeros((2,) + pafs.shape[1:])
    for paf in pafs.reshape((pafs.shape[0] // 2, 2) + pafs.shape[1:]):
        mix += paf
    return mix


def overlay_pafs_np(img, pafs):
    """overlay_pafs (:39-50).  The reference reads as an average over the limbs present at a pixel,
    but ``paf_flags`` is rebound on every iteration (:44, ``paf_flags = paf != 0``) and the in-place
    ``+=`` of the broadcast (:45) keeps it boolean, so :48 divides by ``True``: the mix is the plain
    float64 sum of the limbs.  That is what it shows, and what this states."""
    return overlay_paf_np(img, mix_pafs_np(pafs))


def jet_index_np(heatmap):
    """The index image ``overlay_heatmap`` (:53) hands to ``cv2.applyColorMap``: ``heatmap * 255`` in
    float32, truncated.  The clip to 0 .. 255 is this package's addition: label maps lie in [0, 1],
    network maps overshoot, and ``astype(uint8)`` of a negative float is not defined."""
    return np.clip(np.asarray(heatmap, f32) * f32(255.0), f32(0.0), f32(255.0)).astype(np.uint8)


def overlay_heatmap_np(img, heatmap, lut=None):
    """overlay_heatmap (:52-55): heatmap float32 (h, w) through ``lut`` (default ``jet_lut()``)."""
    return add_weighted(img, 0.6, _lut(lut)[jet_index_np(heatmap)], 0.4, 0)


def overlay_ignore_mask_np(img, mask):
    """overlay_ignore_mask (:57-59): img * (mask == 0)."""
    return img * np.repeat((np.asarray(mask) == 0).astype(np.uint8)[:, :, None], 3, axis=2)


def _finite(name, maps):
    if maps is not None and not np.all(np.isfinite(maps)):
        raise ValueError("overlay: %s hold a value that is not finite" % name)


def _as_frame(img, pafs, heatmaps, ignore_mask):
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or min(img.shape[:2]) < 1:
        raise ValueError("overlay: an (h, w, 3) uint8 image expected")
    if pafs is not None:
        pafs = np.asarray(pafs, f32)
        if pafs.ndim != 3 or pafs.shape[0] < 2 or pafs.shape[0] % 2 or min(pafs.shape[1:]) < 1:
            raise ValueError("overlay: pafs (2L, mh, mw) expected, got %s" % (pafs.shape,))
        _finite("pafs", pafs)
    if heatmaps is not None:
        heatmaps = np.asarray(heatmaps, f32)
        if heatmaps.ndim != 3 or min(heatmaps.shape) < 1:
            raise ValueError("overlay: heatmaps (C, mh, mw) expected, got %s" % (heatmaps.shape,))
        _finite("heatmaps", heatmaps)
    if ignore_mask is not None:
        ignore_mask = np.asarray(ignore_mask) != 0
        if ignore_mask.ndim != 2 or min(ignore_mask.shape) < 1:
            raise ValueError("overlay: ignore_mask (h, w) expected, got %s" % (ignore_mask.shape,))
    return img, pafs, heatmaps, ignore_mask


def overlay_np(img, pafs=None, heatmaps=None, ignore_mask=None, lut=None):
    """The viewer's sequence (:372-382) and the statement the device is held to: whichever layers are
    given, in the order PAFs, heat, mask.  pafs (2L, mh, mw) and heatmaps (C, mh, mw) are resized to
    the frame (``resize_linear_f32_np``); the heat shown is the float32 maximum over the channels
    passed (the reference passes ``heatmaps[:-1]``: ``overlay_labels_np``); ignore_mask, nonzero =
    ignored at any size, is resized as ``cv2.resize(mask.astype(np.uint8) * 255, shape) > 0``."""
    img, pafs, heatmaps, ignore_mask = _as_frame(img, pafs, heatmaps, ignore_mask)
    lut = _lut(lut)
    h, w = img.shape[:2]
    out = img.copy()
    if pafs is not None:
        out = overlay_pafs_np(out, resize_linear_f32_np(pafs, h, w))
    if heatmaps is not None:
        out = overlay_heatmap_np(out, resize_linear_f32_np(heatmaps, h, w).max(axis=0), lut)
    if ignore_mask is not None:
        out = overlay_ignore_mask_np(out, resize_linear_np(ignore_mask.astype(np.uint8) * 255, w, h) > 0)
    return out


def overlay_labels_np(img, pafs, heatmaps, ignore_mask):
    """A training sample's picture (:379-382): the background heat map is left out."""
    return overlay_np(img, pafs, heatmaps[:-1], ignore_mask)


# ---- the device ----
def _per_frame(name, v, n):
    if v is None:
        return [None] * n
    if len(v) != n:
        raise ValueError("overlay: one %s entry per frame expected" % name)
    return list(v)


def overlay(imgs, pafs=None, heatmaps=None, ignore_masks=None, lut=None, device=0):
    """``overlay_np`` for a batch on the device (op_overlay): imgs n arrays (h_i, w_i, 3) uint8 of any
    sizes; pafs, heatmaps, ignore_masks None or n entries, each None or that frame's layer.  One kernel
    launch; returns the n pictures."""
    n = len(imgs)
    if n < 1:
        raise ValueError("overlay: n >= 1 images expected")
    lut = _lut(lut)
    frames = [_as_frame(imgs[i], p, t, m) for i, (p, t, m) in enumerate(zip(
        _per_frame("pafs", pafs, n), _per_frame("heatmaps", heatmaps, n), _per_frame("ignore_masks", ignore_masks, n)))]
    keep = [_lib._row_strided_u8(f[0]) for f in frames]
    outs = [np.empty(a.shape, np.uint8) for a in keep]

    def layer(k, dtype):
        arrs = [None if f[k] is None else np.ascontiguousarray(f[k], dtype) for f in frames]
        if all(a is None for a in arrs):
            return arrs, None, None
        dims = np.zeros((n, 3 if dtype == f32 else 2), np.int32)
        for i, a in enumerate(arrs):
            if a is not None:
                dims[i] = a.shape
        return arrs, (ctypes.c_void_p * n)(*[None if a is None else a.ctypes.data for a in arrs]), dims

    kp, pp, pd = layer(1, f32)  # (kp, kh, km hold what the pointers point to until the call returns)
    kh, hp, hd = layer(2, f32)
    km, mp, md = layer(3, np.uint8)
    bgr = (ctypes.c_void_p * n)(*[a.ctypes.data for a in keep])
    out = (ctypes.c_void_p * n)(*[a.ctypes.data for a in outs])
    strides = np.array([a.strides[0] for a in keep], np.int64)
    hw = np.array([a.shape[:2] for a in keep], np.int32)
    _lib.check(_lib.lib().op_overlay(int(device), n, bgr, _lib.ptr(strides), _lib.ptr(hw), pp, _lib.ptr(pd), hp,
                                     _lib.ptr(hd), mp, _lib.ptr(md), _lib.ptr(lut), out), "op_overlay")
    return outs


def overlay_labels(imgs, pafs, heatmaps, ignore_masks, device=0):
    """``overlay_labels_np`` for a batch on the device: what ``labels.make_labels`` returns over the
    frames it was made for."""
    return overlay(imgs, pafs, [t[:-1] for t in heatmaps], ignore_masks, device=device)


def overlay_staged(ctx, first, n, pafs=True, heatmaps=True, lut=None):
    """The same kernel on staged frames [first, first + n) of the ``_lib.Context`` ``ctx`` and the
    network maps ``ctx.fetch_maps`` would return for them, all read in place on the device
    (op_overlay_staged): the last-stage maps after ``run_staged``, the averaged full-resolution maps
    after ``run_staged_precise``.  Heat shows the 18 joint channels.  It runs behind a queued run and
    modifies nothing.  Returns (n, h, w, 3) uint8."""
    layers = (OP_OVERLAY_PAFS if pafs else 0) | (OP_OVERLAY_HEAT if heatmaps else 0)
    lut = _lut(lut)
    _, h, w = ctx.staged_info()
    out = np.empty(max(n, 1) * max(h * w * 3, 1), np.uint8)  # nothing staged: the call itself says so
    _lib.check(_lib.lib().op_overlay_staged(ctx.h, int(first), int(n), layers, _lib.ptr(lut), _lib.ptr(out)),
               "op_overlay_staged")
    return out.reshape(n, h, w, 3)


def last_ms(device=0):
    """Device time (uploads + kernel, stream events) of the last ``overlay`` / ``overlay_staged`` that
    completed on this device."""
    ms = ctypes.c_double()
    _lib.check(_lib.lib().op_overlay_last_ms(int(device), ctypes.byref(ms)), "op_overlay_last_ms")
    return ms.value
