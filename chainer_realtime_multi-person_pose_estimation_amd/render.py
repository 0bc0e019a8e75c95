"""Skeleton overlays on the device: the drawing of ``draw.py`` / ``demo.run`` as a display list.

The work is split into a list and pixels.  ``DisplayList`` is a recording ``draw.Raster``: run under
it, the unchanged ``draw.draw_person_pose`` makes its ``line`` / ``circle`` calls (the sequence
tests/golden/draw_calls.json pins to the reference's own) and every call becomes a primitive:

    LINE(x0, y0, x1, y1, thickness, color)   float64 end points and thickness
    DISC(x, y, radius, color)                integer centre and radius
    BLEND(wa, wb, gamma)                     at most one per list

``color`` is BGR uint8, rounded as ``draw._paint`` rounds it.  The order is painter's order: a later
primitive overwrites an earlier one.  ``BLEND`` turns the picture so far into
``demo.add_weighted(input, wa, picture, wb, gamma)``; the primitives after it paint over the blend,
so all of ``demo.run``'s drawing is one list (``demo_list``).

``render_np`` executes a list with ``draw.draw_line``, ``draw.draw_disc`` and ``demo.add_weighted``
and nothing else: it is the statement.  ``render`` / ``render_staged`` execute lists for a batch of
frames in one kernel launch (op_draw / op_draw_staged, csrc/draw.hip) and agree with ``render_np``
bit for bit.  ``draw.py``'s rasteriser itself stays unpinned against OpenCV's, as before.
"""
import collections
import ctypes

import numpy as np

from . import _lib
from . import draw as _draw
from .constants import params
from .hand_detector import FINGER_COLORS

LINE = collections.namedtuple("LINE", "x0 y0 x1 y1 thickness color")
DISC = collections.namedtuple("DISC", "x y radius color")
BLEND = collections.namedtuple("BLEND", "wa wb gamma")

FACE_COLOR = (255, 255, 0)
RECT_COLOR = (255, 255, 255)
DEMO_BLEND = BLEND(0.6, 0.4, 0.0)  # demo.run / pose_detector.py:575: cv2.addWeighted(img, 0.6, pose, 0.4, 0)


def _color(color):
    """The three bytes ``draw._paint`` stores for ``color``."""
    c = np.asarray(color, np.float64).round().astype(np.uint8)
    if c.shape != (3,):
        raise ValueError("render: a colour is three BGR values, got %r" % (color,))
    return (int(c[0]), int(c[1]), int(c[2]))


def line_prim(pt1, pt2, color, thickness):
    (x0, y0), (x1, y1) = pt1, pt2
    return LINE(float(x0), float(y0), float(x1), float(y1), float(thickness), _color(color))


def disc_prim(center, radius, color):
    x, y = center
    if int(x) != x or int(y) != y or int(radius) != radius:
        raise ValueError("render: a disc has an integer centre and radius, got %r, %r" % (center, radius))
    return DISC(int(x), int(y), int(radius), _color(color))


class DisplayList(_draw.Raster):
    """A ``draw.Raster`` that records its calls as primitives (``prims``) and paints nothing."""

    def __init__(self):
        self.prims = []

    def line(self, img, pt1, pt2, color, thickness):
        self.prims.append(line_prim(pt1, pt2, color, thickness))

    def circle(self, img, center, radius, color, thickness):
        if thickness >= 0:
            raise ValueError("render.DisplayList.circle: only filled discs (thickness -1) are drawn")
        self.prims.append(disc_prim(center, radius, color))


def pose_list(poses):
    """The primitives ``draw.draw_person_pose(img, poses)`` paints, in its order."""
    dl = DisplayList()
    _draw.draw_person_pose(np.zeros((1, 1, 3), np.uint8), poses, raster=dl)
    return dl.prims


def calls(prims):
    """The ``line`` / ``circle`` calls a list stands for, as tests/golden/draw_calls.json records them
    (without its ``canvas`` entry)."""
    out = []
    for p in prims:
        if isinstance(p, LINE):
            out.append({"op": "line", "pt1": [int(p.x0), int(p.y0)], "pt2": [int(p.x1), int(p.y1)],
                        "color": [float(v) for v in p.color], "thickness": int(p.thickness)})
        elif isinstance(p, DISC):
            out.append({"op": "circle", "center": [p.x, p.y], "radius": p.radius,
                        "color": [float(v) for v in p.color], "thickness": -1})
        else:
            raise ValueError("render.calls: %r is no line or disc" % (p,))
    return out


def face_list(face_keypoints, left_top):
    """``face_detector.draw_face_keypoints``: its discs and lines, with its coordinate arithmetic."""
    left, top = left_top
    prims = []
    for kp in face_keypoints:
        if kp:
            x, y, _ = kp
            prims.append(disc_prim((int(x + left), int(y + top)), 2, FACE_COLOR))
    for a, b in params["face_line_indices"]:
        ka, kb = face_keypoints[a], face_keypoints[b]
        if ka and kb:
            prims.append(line_prim((ka[0] + left, ka[1] + top), (kb[0] + left, kb[1] + top), FACE_COLOR, 1))
    return prims


def hand_list(hand_keypoints, left_top):
    """``hand_detector.draw_hand_keypoints``: its discs and lines, with its coordinate arithmetic."""
    left, top = left_top
    prims = []
    for i, finger in enumerate(params["fingers_indices"]):
        for a, b in finger:
            ka, kb = hand_keypoints[a], hand_keypoints[b]
            if ka:
                prims.append(disc_prim((int(ka[0] + left), int(ka[1] + top)), 3, FINGER_COLORS[i]))
            if kb:
                prims.append(disc_prim((int(kb[0] + left), int(kb[1] + top)), 3, FINGER_COLORS[i]))
            if ka and kb:
                prims.append(line_prim((ka[0] + left, ka[1] + top), (kb[0] + left, kb[1] + top), FINGER_COLORS[i], 1))
    return prims


def rectangle_list(p0, p1, color):
    """``demo.draw_rectangle``: the four 1-px edges."""
    (x0, y0), (x1, y1) = p0, p1
    return [line_prim(a, b, color, 1) for a, b in
            (((x0, y0), (x1, y0)), ((x1, y0), (x1, y1)), ((x1, y1), (x0, y1)), ((x0, y1), (x0, y0)))]


def demo_list(poses, faces, hands):
    """All of ``demo.run``'s drawing as one list: the pose lines and discs, ``BLEND(0.6, 0.4, 0)``, then
    per person the face keypoints and crop rectangle and the left and right hand alike.  ``faces``
    has per person ``None`` or ``(keypoints, bbox)``; ``hands`` per person a dict with ``"left"`` and
    ``"right"``, each ``None`` or ``(keypoints, bbox)``; bbox = (left, top, right, bottom)."""
    if len(faces) != len(poses) or len(hands) != len(poses):
        raise ValueError("render.demo_list: one faces and one hands entry per person expected")
    prims = pose_list(poses) + [DEMO_BLEND]
    for face, person_hands in zip(faces, hands):
        if face is not None:
            kps, bbox = face
            prims += face_list(kps, (bbox[0], bbox[1]))
            prims += rectangle_list((bbox[0], bbox[1]), (bbox[2], bbox[3]), RECT_COLOR)
        for side in ("left", "right"):
            if person_hands.get(side) is not None:
                kps, bbox = person_hands[side]
                prims += hand_list(kps, (bbox[0], bbox[1]))
                prims += rectangle_list((bbox[0], bbox[1]), (bbox[2], bbox[3]), RECT_COLOR)
    return prims


def render_np(img, prims):
    """The statement: ``prims`` executed on a copy of ``img`` (h, w, 3) uint8 with ``draw.draw_line``,
    ``draw.draw_disc`` and ``demo.add_weighted``."""
    from .demo import add_weighted
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("render_np: an (h, w, 3) uint8 image expected")
    canvas = img.copy()
    blended = False
    for p in prims:
        if isinstance(p, LINE):
            _draw.draw_line(canvas, (p.x0, p.y0), (p.x1, p.y1), p.color, p.thickness)
        elif isinstance(p, DISC):
            _draw.draw_disc(canvas, (p.x, p.y), p.radius, p.color)
        elif isinstance(p, BLEND):
            if blended:
                raise ValueError("render_np: more than one BLEND in a list")
            blended = True
            canvas = add_weighted(img, p.wa, canvas, p.wb, p.gamma)
        else:
            raise ValueError("render_np: unknown primitive %r" % (p,))
    return canvas


# ---- the device ----
def pack_prim(p):
    """One primitive as the C ABI's op_draw_prim."""
    c = _lib.OpDrawPrim()
    if isinstance(p, LINE):
        c.kind = _lib.OP_DRAW_LINE
        c.x0, c.y0, c.x1, c.y1, c.thickness = p.x0, p.y0, p.x1, p.y1, p.thickness
    elif isinstance(p, DISC):
        c.kind = _lib.OP_DRAW_DISC
        c.x0, c.y0, c.radius = p.x, p.y, p.radius
    elif isinstance(p, BLEND):
        c.kind = _lib.OP_DRAW_BLEND
        c.wa, c.wb, c.gamma = p.wa, p.wb, p.gamma
        return c
    else:
        raise ValueError("render: unknown primitive %r" % (p,))
    c.bgr[0], c.bgr[1], c.bgr[2] = p.color
    return c


def pack_lists(lists):
    """-> (prim_offsets int32 [n + 1], op_draw_prim array) of n lists."""
    offsets = np.zeros(len(lists) + 1, np.int32)
    offsets[1:] = np.cumsum([len(l) for l in lists])
    flat = [pack_prim(p) for l in lists for p in l]
    return offsets, (_lib.OpDrawPrim * max(len(flat), 1))(*flat)


def render(imgs, lists, device=0):
    """``render_np`` for a batch on the device (op_draw): imgs n arrays (h_i, w_i, 3) uint8 of any
    sizes, lists n display lists.  One kernel launch; returns the n drawn images."""
    n = len(imgs)
    if n < 1 or len(lists) != n:
        raise ValueError("render: n >= 1 images and as many lists expected")
    keep = []
    for img in imgs:
        img = np.asarray(img)
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("render: (h, w, 3) uint8 images expected")
        keep.append(np.ascontiguousarray(img))
    outs = [np.empty_like(a) for a in keep]
    bgr = (ctypes.c_void_p * n)(*[a.ctypes.data for a in keep])
    out = (ctypes.c_void_p * n)(*[a.ctypes.data for a in outs])
    strides = np.array([a.shape[1] * 3 for a in keep], np.int64)
    hw = np.array([[a.shape[0], a.shape[1]] for a in keep], np.int32)
    offsets, cprims = pack_lists(lists)
    _lib.check(_lib.lib().op_draw(int(device), n, bgr, _lib.ptr(strides), _lib.ptr(hw), _lib.ptr(offsets), cprims, out),
               "op_draw")
    return outs


def render_staged(ctx, first, n, lists):
    """The same kernel on staged frames [first, first + n) of the ``_lib.Context`` ``ctx``, read in
    place on the device (op_draw_staged; the staged frames are not modified).  It runs behind a queued
    ``run_staged``.  Returns (n, h, w, 3) uint8."""
    if n < 1 or len(lists) != n:
        raise ValueError("render_staged: n >= 1 frames and as many lists expected")
    _, h, w = ctx.staged_info()
    offsets, cprims = pack_lists(lists)
    out = np.empty(max(n * h * w * 3, 1), np.uint8)  # nothing staged: the call itself says so
    rc = _lib.lib().op_draw_staged(ctx.h, int(first), int(n), _lib.ptr(offsets), cprims, _lib.ptr(out))
    _lib.check(rc, "op_draw_staged")
    return out.reshape(n, h, w, 3)


def last_ms(device=0):
    """Device time (uploads + kernel, stream events) of the last ``render`` / ``render_staged`` that
    completed on this device."""
    ms = ctypes.c_double()
    _lib.check(_lib.lib().op_draw_last_ms(int(device), ctypes.byref(ms)), "op_draw_last_ms")
    return ms.value
