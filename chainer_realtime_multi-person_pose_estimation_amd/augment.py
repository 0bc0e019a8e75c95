"""Training-sample augmentation (coco_data_loader.py:60-205): random resize, rotate, crop, optional
colour distortion, optional flip, from annotated frames of any size to the network input.

The work is split into a plan and pixels.  ``draw_plan`` makes every random draw and all pose
arithmetic on the host, in the reference's order and with its int32 truncations (pinned to the
reference's own code by tests/golden/augment/plan_*.npz); the result is an ``AugmentPlan`` and the
output poses.  ``augment`` applies the plans of a batch on the device (op_augment, csrc/augment.hip:
a linear resize, then one fused pass per output pixel: undo the flip, map through the crop window,
take the cubic warp taps from the resized image, distort the colour, store; the rotated image is
never materialised).  ``augment_np`` is the same pixel path in NumPy: integer arithmetic, or f32
with one operation per statement, so that the kernels agree with it bit for bit.

``cv2.resize``, ``cv2.warpAffine``, ``cv2.cvtColor`` and ``cv2.getRotationMatrix2D`` are restated
from OpenCV's sources; OpenCV is not available to pin them against ("parity unpinned").
Two constants differ on purpose, as in the reference: the warp's border is
``saturate_cast<uchar>(127.5)`` = 128, the crop's padding ``(zeros + 127.5).astype('uint8')`` = 127.
"""
import ctypes
import math

import numpy as np

from . import _lib
from .constants import JointType
from .labels import train_params

J = JointType
FLIP_PAIRS = [(J.LeftEye, J.RightEye), (J.LeftEar, J.RightEar), (J.LeftShoulder, J.RightShoulder),
              (J.LeftElbow, J.RightElbow), (J.LeftHand, J.RightHand), (J.LeftWaist, J.RightWaist),
              (J.LeftKnee, J.RightKnee), (J.LeftFoot, J.RightFoot)]
WARP_BORDER = 128  # saturate_cast<uchar>(borderValue = 127.5)
CROP_PAD = 127     # (np.zeros(..., 'uint8') + 127.5).astype('uint8')
MAX_SIDE = 16384   # the warp keeps source coordinates as shorts
COLOUR_RANGE = (10, 40, 30)
AB_BITS, INTER_BITS, COEF_BITS = 10, 5, 15
TAB = 1 << INTER_BITS
f32 = np.float32


class AugmentPlan(object):
    """What one sample's augmentation does, all randomness resolved: source size (h, w), resized
    size (rw, rh), ``degree``, the 2x3 forward matrix ``R`` (float64, after the bounding-box shift),
    rotated size (bw, bh), crop ``offset`` (ox, oy) and copy window (crop[y_from:y_to+1,
    x_from:x_to+1] = rotated[y1:y2+1, x1:x2+1]; x2 < x1 or y2 < y1: nothing is copied),
    ``colour`` None or the signed deltas (dh, ds, dv), ``flip`` and ``insize``."""

    FIELDS = ("h", "w", "rw", "rh", "degree", "R", "bw", "bh", "offset", "x1", "y1", "x2", "y2", "x_from", "y_from",
              "x_to", "y_to", "colour", "flip", "insize")

    def __init__(self, **kw):
        missing = [k for k in self.FIELDS if k not in kw]
        if missing or len(kw) != len(self.FIELDS):
            raise TypeError("AugmentPlan: fields %s expected, missing %s" % (self.FIELDS, missing))
        for k in ("h", "w", "rw", "rh", "bw", "bh", "x1", "y1", "x2", "y2", "x_from", "y_from", "x_to", "y_to", "insize"):
            setattr(self, k, int(kw[k]))
        self.degree = float(kw["degree"])
        self.R = np.array(kw["R"], np.float64).reshape(2, 3)
        self.offset = (int(kw["offset"][0]), int(kw["offset"][1]))
        self.colour = None if kw["colour"] is None else tuple(int(v) for v in kw["colour"])
        self.flip = bool(kw["flip"])

    def window_empty(self):
        return self.x2 < self.x1 or self.y2 < self.y1

    def check(self):
        """ValueError for a plan the pixel path cannot run (what op_augment rejects)."""
        if min(self.h, self.w, self.rw, self.rh, self.bw, self.bh, self.insize) < 1:
            raise ValueError("AugmentPlan: sizes must be >= 1")
        if max(self.rw, self.rh, self.bw, self.bh) > MAX_SIDE:
            raise ValueError("AugmentPlan: rw, rh, bw, bh must not exceed %d" % MAX_SIDE)
        if not np.all(np.isfinite(self.R)):
            raise ValueError("AugmentPlan: non-finite matrix")
        if self.x2 - self.x1 != self.x_to - self.x_from or self.y2 - self.y1 != self.y_to - self.y_from:
            raise ValueError("AugmentPlan: the copy window's two sides differ in size")
        if not self.window_empty() and not (
                0 <= self.x_from and self.x_to < self.insize and 0 <= self.y_from and self.y_to < self.insize
                and 0 <= self.x1 and self.x2 < self.bw and 0 <= self.y1 and self.y2 < self.bh):
            raise ValueError("AugmentPlan: the copy window does not fit insize or the rotated size")
        if self.colour is not None and any(abs(d) > r for d, r in zip(self.colour, COLOUR_RANGE)):
            raise ValueError("AugmentPlan: colour deltas outside +-%s" % (COLOUR_RANGE,))
        return self


def rotation_matrix(center, degree):
    """cv2.getRotationMatrix2D(center, degree, 1) in float64 (angle *= CV_PI / 180)."""
    rad = degree * (math.pi / 180)
    a, b = math.cos(rad), math.sin(rad)
    cx, cy = float(center[0]), float(center[1])
    return np.array([[a, b, (1 - a) * cx - b * cy], [-b, a, b * cx + (1 - a) * cy]], np.float64)


def rotate_geometry(rw, rh, degree):
    """random_rotate_img's geometry (:109-115) for a rw x rh image: (R 2x3 float64 shifted to the
    rotated bounding box, bw, bh)."""
    rad = degree * math.pi / 180
    center = (rw / 2, rh / 2)
    R = rotation_matrix(center, degree)
    bbox = (rw * abs(math.cos(rad)) + rh * abs(math.sin(rad)), rw * abs(math.sin(rad)) + rh * abs(math.cos(rad)))
    R[0, 2] += bbox[0] / 2 - center[0]
    R[1, 2] += bbox[1] / 2 - center[1]
    return R, int(bbox[0] + 0.5), int(bbox[1] + 0.5)


def pose_bboxes(poses):
    """get_pose_bboxes (:61-70): per person (x1, y1, x2, y2) of the visible joints, int32; ValueError
    for a person without a visible joint (the minimum of an empty array)."""
    out = []
    for pose in poses:
        vis = pose[pose[:, 2] > 0]
        out.append([vis[:, 0].min(), vis[:, 1].min(), vis[:, 0].max(), vis[:, 1].max()])
    return np.array(out)


def crop_window(center, insize, bw, bh):
    """random_crop_img's window arithmetic (:140-154) for a crop centre in a bw x bh image: dict of
    offset, x1, y1, x2, y2, x_from, y_from, x_to, y_to."""
    center = np.asarray(center)
    half = (insize - 1) / 2
    offset = (center - half + 0.5).astype("i")
    offset_ = (center + half - (bw - 1, bh - 1) + 0.5).astype("i")
    x1, y1 = (int(v) for v in (center - half + 0.5).astype("i"))
    x2, y2 = (int(v) for v in (center + half + 0.5).astype("i"))
    x1, y1, x2, y2 = max(x1, 0), max(y1, 0), min(x2, bw - 1), min(y2, bh - 1)
    x_from = int(-offset[0]) if offset[0] < 0 else 0
    y_from = int(-offset[1]) if offset[1] < 0 else 0
    x_to = int(insize - offset_[0] - 1) if offset_[0] >= 0 else insize - 1
    y_to = int(insize - offset_[1] - 1) if offset_[1] >= 0 else insize - 1
    return dict(offset=(int(offset[0]), int(offset[1])), x1=x1, y1=y1, x2=x2, y2=y2, x_from=x_from, y_from=y_from,
                x_to=x_to, y_to=y_to)


def flip_poses(poses, width):
    """flip_img's pose part (:178-192), in place: x mirrored, left and right joints swapped."""
    poses[:, :, 0] = width - 1 - poses[:, :, 0]
    for a, b in FLIP_PAIRS:
        tmp = poses[:, a].copy()
        poses[:, a] = poses[:, b]
        poses[:, b] = tmp
    return poses


def draw_plan(poses, h, w, insize, py_random, np_random):
    """augment_data (:195-205) without the pixels: consumes ``py_random`` (a random.Random) and
    ``np_random`` (a np.random.RandomState) in the reference's order and returns (AugmentPlan, output
    poses (people, 18, 3) int32).  ``poses`` is not modified."""
    p = train_params
    poses = np.array(poses, np.int32).reshape(-1, len(JointType), 3)
    # random_resize_img (:81-103); the scaled coordinates truncate into the int32 array
    bb = pose_bboxes(poses)
    sizes = ((bb[:, 2:] - bb[:, :2] + 1) ** 2).sum(axis=1) ** 0.5
    min_scale = min(max(p["min_box_size"] / sizes.min(), p["min_scale"]), 1)
    max_scale = min(max(p["max_box_size"] / sizes.max(), 1), p["max_scale"])
    scale = float((max_scale - min_scale) * py_random.random() + min_scale)
    rw, rh = round(w * scale), round(h * scale)
    poses[:, :, :2] = poses[:, :, :2] * np.array((rw, rh)) / np.array((w, h))
    # random_rotate_img (:105-124)
    degree = np_random.randn() / 3 * p["max_rotate_degree"]
    R, bw, bh = rotate_geometry(rw, rh, degree)
    ones = np.ones_like(poses)
    ones[:, :, :2] = poses[:, :, :2]
    rotated = poses.copy()
    rotated[:, :, :2] = np.dot(ones, R.T)  # truncates again
    poses = rotated
    # random_crop_img (:126-160)
    bb = pose_bboxes(poses)
    box = bb[py_random.choice(range(len(bb)))]
    box_center = box[:2] + (box[2:] - box[:2]) / 2
    perturb = (np_random.rand(2) - 0.5) * 2 * p["center_perterb_max"]
    win = crop_window((box_center + perturb + 0.5).astype("i"), insize, bw, bh)
    poses[:, :, :2] -= np.array(win["offset"], np.int32)
    # distort_color (:162-173) and flip_img (:175-193)
    colour = None
    if np_random.randint(2):
        colour = tuple(int(np_random.randint(2 * r + 1)) - r for r in COLOUR_RANGE)
    flip = bool(np_random.randint(2))
    if flip:
        flip_poses(poses, insize)
    plan = AugmentPlan(h=h, w=w, rw=rw, rh=rh, degree=degree, R=R, bw=bw, bh=bh, colour=colour, flip=flip,
                       insize=insize, **win)
    return plan.check(), poses


# ---- the pixel path in NumPy ----
def _linear_coeffs(dsize, ssize, clamp):
    scale = 1.0 / (float(dsize) / float(ssize))
    f = ((np.arange(dsize, dtype=np.float64) + 0.5) * scale - 0.5).astype(f32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(f32)
    if clamp:
        lo, hi = s < 0, s >= ssize - 1
        f[lo | hi] = 0.0
        s[lo] = 0
        s[hi] = ssize - 1
    c0 = np.clip(np.rint((f32(1.0) - f) * f32(2048.0)).astype(np.int64), -32768, 32767)
    c1 = np.clip(np.rint(f * f32(2048.0)).astype(np.int64), -32768, 32767)
    return s, c0, c1


def resize_linear_np(img, out_w, out_h):
    """cv2.resize(img, (out_w, out_h)), INTER_LINEAR on uint8 (h, w[, c]): OpenCV's fixed-point path,
    11-bit coefficients, int32 horizontal pass, the vertical pass as its SIMD body computes it."""
    img = np.asarray(img, np.uint8)
    src = img.reshape(img.shape[0], img.shape[1], -1).astype(np.int64)
    sh, sw = src.shape[:2]
    sx, a0, a1 = _linear_coeffs(out_w, sw, True)
    sy, b0, b1 = _linear_coeffs(out_h, sh, False)
    x1 = np.minimum(sx + 1, sw - 1)
    hres = src[:, sx] * a0[None, :, None] + src[:, x1] * a1[None, :, None]
    r0, r1 = np.clip(sy, 0, sh - 1), np.clip(sy + 1, 0, sh - 1)
    t0 = ((hres[r0] >> 4) * b0[:, None, None]) >> 16
    t1 = ((hres[r1] >> 4) * b1[:, None, None]) >> 16
    out = np.clip((t0 + t1 + 2) >> 2, 0, 255).astype(np.uint8)
    return out.reshape((out_h, out_w) + img.shape[2:])


def _cubic_coeffs(x):
    """interpolateCubic(x, A = -0.75) in f32: (len(x), 4)."""
    x = np.asarray(x, f32)
    A = f32(-0.75)
    x1 = x + f32(1.0)
    c0 = ((A * x1 - f32(-3.75)) * x1 + f32(-6.0)) * x1 - f32(-3.0)
    c1 = ((f32(1.25) * x - f32(2.25)) * x) * x + f32(1.0)
    y = f32(1.0) - x
    c2 = ((f32(1.25) * y - f32(2.25)) * y) * y + f32(1.0)
    c3 = ((f32(1.0) - c0) - c1) - c2
    return np.stack([c0, c1, c2, c3], axis=1).astype(f32)


def _remap_table(tab1d):
    """initInterTab2D: (1024, k*k) int16 from the (32, k) f32 1-D coefficients; set ay*32 + ax holds
    rows (y taps) of columns (x taps), each ``saturate_cast<short>(v * 32768)``.  A set that does not
    sum to 1 << 15 gets the deficit added to the largest (sum too small) or smallest (sum too large)
    of the taps k/2, k/2 + 1 on each axis: OpenCV's loop bounds, the lower-right 2x2 of the cubic's
    4x4.  A weight of 1.0 saturates to 32767, so the zero-fraction cubic set is 32767 on the pixel
    and 1 on its lower-right neighbour, which still reproduces every uint8 value exactly."""
    k = tab1d.shape[1]
    v = (tab1d[:, None, :, None] * tab1d[None, :, None, :]).astype(f32)  # [ay][ax][ky][kx], one f32 product
    it = np.clip(np.rint(v * f32(1 << COEF_BITS)), -32768, 32767).astype(np.int64).reshape(TAB * TAB, k, k)
    c = k // 2
    for s in it:
        diff = int(s.sum()) - (1 << COEF_BITS)
        if diff == 0:
            continue
        mk = Mk = (c, c)
        for k1 in range(c, min(c + 2, k)):  # (the 2x2 linear sets have the one tap (1, 1) there)
            for k2 in range(c, min(c + 2, k)):
                if s[k1, k2] < s[mk]:
                    mk = (k1, k2)
                elif s[k1, k2] > s[Mk]:
                    Mk = (k1, k2)
        s[Mk if diff < 0 else mk] -= diff
    assert it.min() >= -32768 and it.max() <= 32767
    return it.reshape(TAB * TAB, k * k).astype(np.int16)


_tables = {}


def warp_tables():
    """(cubic (1024, 16) int16, linear (1024, 4) int16): the remap weight tables of warpAffine."""
    if "warp" not in _tables:
        x = np.arange(TAB, dtype=f32) * f32(1.0 / TAB)
        _tables["warp"] = (_remap_table(_cubic_coeffs(x)), _remap_table(np.stack([f32(1.0) - x, x], axis=1)))
    return _tables["warp"]


def hsv_tables():
    """(sdiv (256,), hdiv (256,)) int32 of OpenCV's u8 BGR2HSV with H in 0..180 (hsv_shift = 12)."""
    if "hsv" not in _tables:
        v = np.arange(1, 256, dtype=np.float64)
        sdiv, hdiv = np.zeros(256, np.int32), np.zeros(256, np.int32)
        sdiv[1:] = np.rint((255 << 12) / v)
        hdiv[1:] = np.rint((180 << 12) / (6.0 * v))
        _tables["hsv"] = (sdiv, hdiv)
    return _tables["hsv"]


def _rint_i32(v):
    return np.rint(np.clip(v, -2147483648.0, 2147483647.0)).astype(np.int64)


def _wrap32(v):
    return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)  # int32 sums wrap


def invert_affine(R):
    """warpAffine's inversion of the forward matrix, float64, OpenCV's operation order."""
    M = [float(v) for v in np.asarray(R, np.float64).ravel()]
    D = M[0] * M[4] - M[1] * M[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = M[4] * D, M[0] * D
    M[0] = A11
    M[1] *= -D
    M[3] *= -D
    M[4] = A22
    b1 = -M[0] * M[2] - M[1] * M[5]
    b2 = -M[3] * M[2] - M[4] * M[5]
    M[2], M[5] = b1, b2
    return M


def warp_coords(R, xs, ys):
    """Fixed-point source coordinates of the rotated-image pixels xs (columns) x ys (rows):
    (sx, sy, ax, ay) int64 arrays (len(ys), len(xs)); sx, sy saturate to shorts."""
    M = invert_affine(R)
    xs, ys = np.asarray(xs, np.float64), np.asarray(ys, np.float64)
    scale = float(1 << AB_BITS)
    adelta = _rint_i32(M[0] * xs * scale)
    bdelta = _rint_i32(M[3] * xs * scale)
    rd = (1 << AB_BITS) // TAB // 2
    X0 = _wrap32(_rint_i32((M[1] * ys + M[2]) * scale) + rd)
    Y0 = _wrap32(_rint_i32((M[4] * ys + M[5]) * scale) + rd)
    X = _wrap32(X0[:, None] + adelta[None, :]) >> (AB_BITS - INTER_BITS)
    Y = _wrap32(Y0[:, None] + bdelta[None, :]) >> (AB_BITS - INTER_BITS)
    return (np.clip(X >> INTER_BITS, -32768, 32767), np.clip(Y >> INTER_BITS, -32768, 32767),
            X & (TAB - 1), Y & (TAB - 1))


def warp_affine_np(img, mask, R, xs, ys):
    """The pixels xs x ys of ``cv2.warpAffine(img, R, (bw, bh), INTER_CUBIC, BORDER_CONSTANT, 127.5)``
    and of ``cv2.warpAffine(mask * 255, R, (bw, bh)) > 0``: img (rh, rw, 3) u8, mask (rh, rw) bool."""
    cub, lin = warp_tables()
    rh, rw = img.shape[:2]
    sx, sy, ax, ay = warp_coords(R, xs, ys)
    sel = ay * TAB + ax
    src = img.astype(np.int64)
    acc = np.zeros(sx.shape + (3,), np.int64)
    wc = cub[sel].astype(np.int64)
    for ky in range(4):
        for kx in range(4):
            x, y = sx - 1 + kx, sy - 1 + ky
            inside = (x >= 0) & (x < rw) & (y >= 0) & (y < rh)
            tap = np.where(inside[..., None], src[np.clip(y, 0, rh - 1), np.clip(x, 0, rw - 1)], WARP_BORDER)
            acc += tap * wc[..., ky * 4 + kx, None]
    out = np.clip((acc + (1 << (COEF_BITS - 1))) >> COEF_BITS, 0, 255).astype(np.uint8)
    m255 = np.asarray(mask, bool).astype(np.int64) * 255
    macc = np.zeros(sx.shape, np.int64)
    wl = lin[sel].astype(np.int64)
    for ky in range(2):
        for kx in range(2):
            x, y = sx + kx, sy + ky
            inside = (x >= 0) & (x < rw) & (y >= 0) & (y < rh)
            macc += np.where(inside, m255[np.clip(y, 0, rh - 1), np.clip(x, 0, rw - 1)], 0) * wl[..., ky * 2 + kx]
    return out, np.clip((macc + (1 << (COEF_BITS - 1))) >> COEF_BITS, 0, 255) > 0


def bgr2hsv_np(img):
    """cv2.cvtColor(img, COLOR_BGR2HSV) on uint8, OpenCV's integer path (H in 0..180) -> int32."""
    sdiv, hdiv = hsv_tables()
    x = np.asarray(img, np.uint8).astype(np.int64)
    b, g, r = x[..., 0], x[..., 1], x[..., 2]
    v = np.maximum(np.maximum(b, g), r)
    diff = v - np.minimum(np.minimum(b, g), r)
    s = (diff * sdiv[v] + (1 << 11)) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * hdiv[diff] + (1 << 11)) >> 12
    h = h + np.where(h < 0, 180, 0)
    return np.stack([np.clip(h, 0, 255), s & 255, v], axis=-1).astype(np.int32)


_SECTOR = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])


def hsv2bgr_np(hsv):
    """cv2.cvtColor(hsv, COLOR_HSV2BGR) on uint8: OpenCV's float path, one f32 operation per
    statement, ``* 255`` rounded half-to-even and saturated."""
    x = np.asarray(hsv, np.uint8).astype(f32)
    h = x[..., 0] * (f32(6.0) / f32(180.0))
    s = x[..., 1] * (f32(1.0) / f32(255.0))
    v = x[..., 2] * (f32(1.0) / f32(255.0))
    while np.any(h >= f32(6.0)):
        h = np.where(h >= f32(6.0), h - f32(6.0), h)
    sector = np.floor(h).astype(np.int64)
    h = h - sector.astype(f32)
    t1 = f32(1.0) - s
    t1 = v * t1
    t2 = s * h
    t2 = f32(1.0) - t2
    t2 = v * t2
    t3 = f32(1.0) - h
    t3 = s * t3
    t3 = f32(1.0) - t3
    t3 = v * t3
    tab = np.stack([v, t1, t2, t3], axis=-1)
    bgr = np.take_along_axis(tab, _SECTOR[sector], axis=-1)
    bgr = np.where((x[..., 1] == 0)[..., None], v[..., None], bgr)
    return np.clip(np.rint(bgr * f32(255.0)), 0, 255).astype(np.uint8)


def distort_colour_np(img, colour):
    """distort_color (:162-173) with the drawn deltas: BGR2HSV, the int32 clip(channel + delta, 0,
    255) on all three channels (hue does not wrap), HSV2BGR."""
    hsv = bgr2hsv_np(img)
    hsv = np.maximum(np.minimum(hsv + np.array(colour, np.int32), 255), 0)
    return hsv2bgr_np(hsv.astype(np.uint8))


def _as_sample(img, mask, plan):
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.shape != (plan.h, plan.w, 3):
        raise ValueError("augment: image (%d, %d, 3) uint8 expected, got %s %s" % (plan.h, plan.w, img.shape, img.dtype))
    if mask is not None:
        mask = np.asarray(mask) != 0
        if mask.shape != (plan.h, plan.w):
            raise ValueError("augment: mask (%d, %d) expected, got %s" % (plan.h, plan.w, mask.shape))
    return img, mask


def augment_np(img, mask, plan):
    """The plan's pixel path on the host: img (h, w, 3) u8 BGR, mask (h, w) nonzero = ignored or
    None -> ((insize, insize, 3) u8, (insize, insize) bool)."""
    plan.check()
    img, mask = _as_sample(img, mask, plan)
    n = plan.insize
    out = np.full((n, n, 3), CROP_PAD, np.uint8)
    omask = np.zeros((n, n), bool)
    if not plan.window_empty():
        small = resize_linear_np(img, plan.rw, plan.rh)
        msmall = resize_linear_np(mask.astype(np.uint8), plan.rw, plan.rh) != 0 if mask is not None \
            else np.zeros((plan.rh, plan.rw), bool)
        win, mwin = warp_affine_np(small, msmall, plan.R, np.arange(plan.x1, plan.x2 + 1),
                                   np.arange(plan.y1, plan.y2 + 1))
        out[plan.y_from:plan.y_to + 1, plan.x_from:plan.x_to + 1] = win
        omask[plan.y_from:plan.y_to + 1, plan.x_from:plan.x_to + 1] = mwin
    if plan.colour is not None:
        out = distort_colour_np(out, plan.colour)
    if plan.flip:
        out, omask = out[:, ::-1], omask[:, ::-1]
    return np.ascontiguousarray(out), np.ascontiguousarray(omask)


# ---- the device ----
class OpAugmentPlan(ctypes.Structure):
    """op_augment_plan (include/openpose_hip.h)."""
    _fields_ = [("h", ctypes.c_int32), ("w", ctypes.c_int32), ("rw", ctypes.c_int32), ("rh", ctypes.c_int32),
                ("degree", ctypes.c_double), ("R", ctypes.c_double * 6), ("bw", ctypes.c_int32), ("bh", ctypes.c_int32),
                ("ox", ctypes.c_int32), ("oy", ctypes.c_int32), ("x1", ctypes.c_int32), ("y1", ctypes.c_int32),
                ("x2", ctypes.c_int32), ("y2", ctypes.c_int32), ("x_from", ctypes.c_int32), ("y_from", ctypes.c_int32),
                ("x_to", ctypes.c_int32), ("y_to", ctypes.c_int32), ("colour", ctypes.c_int32), ("dh", ctypes.c_int32),
                ("ds", ctypes.c_int32), ("dv", ctypes.c_int32), ("flip", ctypes.c_int32), ("insize", ctypes.c_int32)]


def pack_plan(plan):
    c = plan.colour or (0, 0, 0)
    return OpAugmentPlan(plan.h, plan.w, plan.rw, plan.rh, plan.degree, (ctypes.c_double * 6)(*plan.R.ravel()), plan.bw,
                         plan.bh, plan.offset[0], plan.offset[1], plan.x1, plan.y1, plan.x2, plan.y2, plan.x_from,
                         plan.y_from, plan.x_to, plan.y_to, int(plan.colour is not None), c[0], c[1], c[2],
                         int(plan.flip), plan.insize)


def augment(imgs, masks, plans, device=0):
    """``augment_np`` for a batch on the device (op_augment): imgs n arrays (h_i, w_i, 3) u8, masks
    None or n entries (array or None), plans n AugmentPlans of one insize.  Returns (imgs (n, insize,
    insize, 3) u8, masks (n, insize, insize) bool)."""
    n = len(plans)
    if n < 1 or len(imgs) != n or (masks is not None and len(masks) != n):
        raise ValueError("augment: n >= 1 images, plans and (optionally) masks expected")
    insize = plans[0].insize
    keep, mkeep = [], []
    for i in range(n):
        img, mask = _as_sample(imgs[i], masks[i] if masks is not None else None, plans[i])
        keep.append(np.ascontiguousarray(img))
        mkeep.append(None if mask is None else np.ascontiguousarray(mask, np.uint8))
    bgr = (ctypes.c_void_p * n)(*[a.ctypes.data for a in keep])
    strides = np.array([a.shape[1] * 3 for a in keep], np.int64)
    mk = (ctypes.c_void_p * n)(*[None if a is None else a.ctypes.data for a in mkeep]) if masks is not None else None
    cplans = (OpAugmentPlan * n)(*[pack_plan(p) for p in plans])
    out = np.empty((n, insize, insize, 3), np.uint8)
    omask = np.empty((n, insize, insize), np.uint8)
    _lib.check(_lib.lib().op_augment(int(device), n, bgr, _lib.ptr(strides), mk, cplans, int(insize), _lib.ptr(out),
                                     _lib.ptr(omask)), "op_augment")
    return out, omask.astype(bool)


def last_ms(device=0):
    """Device time (uploads + kernels, stream events) of the last ``augment`` on this device."""
    ms = ctypes.c_double()
    _lib.check(_lib.lib().op_augment_last_ms(int(device), ctypes.byref(ms)), "op_augment_last_ms")
    return ms.value


def last_paths(device=0):
    """(pixels warped from the LDS-staged box, pixels warped from global memory) in the last
    ``augment`` on this device; pixels outside their crop window count in neither."""
    c = np.zeros(2, np.int64)
    _lib.check(_lib.lib().op_augment_last_paths(int(device), _lib.ptr(c)), "op_augment_last_paths")
    return int(c[0]), int(c[1])


def device_tables():
    """The library's own host-built tables (cubic, linear, sdiv, hdiv), as ``warp_tables`` and
    ``hsv_tables`` give them: what the kernels read."""
    cub, lin = np.empty((TAB * TAB, 16), np.int16), np.empty((TAB * TAB, 4), np.int16)
    sdiv, hdiv = np.empty(256, np.int32), np.empty(256, np.int32)
    _lib.check(_lib.lib().op_augment_tables(_lib.ptr(cub), _lib.ptr(lin), _lib.ptr(sdiv), _lib.ptr(hdiv)),
               "op_augment_tables")
    return cub, lin, sdiv, hdiv


def augment_batch(samples, insize, py_random, np_random, device=0):
    """The loader's body for a batch: samples = [(img (h, w, 3) u8, mask (h, w) or None, poses
    (people, 18, 3))] of any sizes -> (imgs (n, insize, insize, 3) u8, poses_per_frame, mask (n,
    insize, insize) bool), the arguments of ``Updater.update_poses``."""
    plans, poses = [], []
    for img, mask, p in samples:
        plan, out = draw_plan(p, img.shape[0], img.shape[1], insize, py_random, np_random)
        plans.append(plan)
        poses.append(out)
    imgs, mask = augment([s[0] for s in samples], [s[1] for s in samples], plans, device)
    return imgs, poses, mask
