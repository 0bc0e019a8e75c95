"""Training labels from COCO keypoint annotations (coco_data_loader.py:208-341).

``make_labels`` runs on the device (op_make_labels, csrc/labels.hip): part-affinity fields, heat
maps and the dilated ignore mask of a batch of frames, at full resolution (``downscale=1``, what
the reference's ``generate_pafs`` / ``generate_heatmaps`` return) or at the network map size
(``downscale=8``: what ``compute_loss`` makes of them with ``F.resize_images``, evaluated at the
four bilinear taps of every output pixel only).  ``make_labels_np`` is the same computation in
float64 NumPy on the host: the path for a machine without the device, and the check of the kernel.

``train_params`` holds the training entries of the reference's params dict (entity.py:56-68) and
its ``coco_joint_indices`` (entity.py:106-124); ``parse_coco_annotation`` / ``valid_annotations``
turn the person annotations of a COCO keypoints JSON (plain dicts, no pycocotools) into the
integer-valued (people, 18, 3) pose arrays the labels are made from.  Image-side augmentation (the
cv2 warps and colour distortion of coco_data_loader.py:60-205) is augment.py: ``augment_batch``
turns annotated frames of any size into the images, poses and mask these labels are made from.
"""
import numpy as np

from . import _lib
from .constants import JointType, params

J = JointType
train_params = dict(
    min_keypoints=5,
    min_area=32 * 32,
    insize=368,
    downscale=8,
    paf_sigma=8,
    heatmap_sigma=7,
    min_box_size=64,
    max_box_size=512,
    min_scale=0.5,
    max_scale=2.0,
    max_rotate_degree=40,
    center_perterb_max=40,
    # COCO's 17 keypoints in annotation order -> JointType (the Neck is computed)
    coco_joint_indices=[J.Nose, J.LeftEye, J.RightEye, J.LeftEar, J.RightEar, J.LeftShoulder, J.RightShoulder,
                        J.LeftElbow, J.RightElbow, J.LeftHand, J.RightHand, J.LeftWaist, J.RightWaist, J.LeftKnee,
                        J.RightKnee, J.LeftFoot, J.RightFoot],
)
DILATE = 16  # cv2.morphologyEx(mask, cv2.MORPH_DILATE, np.ones((16, 16))), coco_data_loader.py:340


def valid_annotations(annotations):
    """The person annotations get_img_annotation keeps (coco_data_loader.py:284-288): enough
    keypoints and a large enough area.  None when none is left, as there."""
    keep = [a for a in annotations
            if a["num_keypoints"] >= train_params["min_keypoints"] and a["area"] > train_params["min_area"]]
    return keep or None


def parse_coco_annotation(annotations):
    """coco_data_loader.py:311-332: (people, 18, 3) int32 poses (x, y, visibility) from the
    ``keypoints`` lists; the Neck is the truncated midpoint of the shoulders when both are labelled."""
    poses = np.zeros((len(annotations), len(JointType), 3), np.int32)
    for pose, ann in zip(poses, annotations):
        pose[train_params["coco_joint_indices"]] = np.array(ann["keypoints"]).reshape(-1, 3)
        ls, rs = pose[J.LeftShoulder], pose[J.RightShoulder]
        if ls[2] > 0 and rs[2] > 0:
            pose[J.Neck] = int((ls[0] + rs[0]) / 2), int((ls[1] + rs[1]) / 2), 2
    return poses


def _out_size(h, w, downscale):
    d = int(downscale)
    if d < 1 or (d > 1 and (h % d or w % d or h // d < 2 or w // d < 2)):
        raise ValueError("downscale %r: 1, or a divisor of h and w with h/downscale, w/downscale >= 2" % (downscale,))
    return h // d, w // d


def make_labels(poses_per_frame, h, w, mask=None, downscale=8, device=0,
                heatmap_sigma=train_params["heatmap_sigma"], paf_width=train_params["paf_sigma"]):
    """Labels of a batch on the device: poses_per_frame = n arrays (people, 18, 3); mask (n, h, w)
    nonzero = ignored, or None.  Returns (pafs (n,38,oh,ow) f32, heatmaps (n,19,oh,ow) f32,
    ignore_mask (n,oh,ow) bool), oh x ow = (h, w) / downscale."""
    n = len(poses_per_frame)
    poses, offsets = _lib.pack_poses(poses_per_frame)
    mk = _lib.pack_mask(mask, n, h, w)
    oh, ow = _out_size(h, w, downscale)
    pafs = np.empty((n, _lib.N_PAF, oh, ow), np.float32)
    heat = np.empty((n, _lib.N_HEAT, oh, ow), np.float32)
    ign = np.empty((n, oh, ow), np.uint8)
    _lib.check(_lib.lib().op_make_labels(int(device), n, int(h), int(w), int(downscale), _lib.ptr(poses),
                                         _lib.ptr(offsets), _lib.ptr(mk), float(heatmap_sigma), float(paf_width),
                                         _lib.ptr(pafs), _lib.ptr(heat), _lib.ptr(ign)), "op_make_labels")
    return pafs, heat, ign.astype(bool)


# ---- the same labels in float64 NumPy ----
def heatmaps_np(poses, h, w, sigma):
    """generate_heatmaps (coco_data_loader.py:216-229) for one frame: (19, h, w) float64."""
    gy, gx = np.mgrid[0:h, 0:w].astype(np.float64)
    poses = np.asarray(poses, np.float64).reshape(-1, len(JointType), 3)
    out = np.zeros((len(JointType) + 1, h, w))
    for j in range(len(JointType)):
        for pose in poses:
            if pose[j, 2] > 0:
                d = (gx - pose[j, 0]) ** 2 + (gy - pose[j, 1]) ** 2
                np.maximum(out[j], np.exp(-0.5 * d / float(sigma) ** 2), out=out[j])
    out[-1] = 1 - out[:-1].max(axis=0)
    return out


def pafs_np(poses, h, w, paf_width):
    """generate_pafs (coco_data_loader.py:232-268) for one frame: (38, h, w) float64."""
    gy, gx = np.mgrid[0:h, 0:w].astype(np.float64)
    poses = np.asarray(poses, np.float64).reshape(-1, len(JointType), 3)
    c, s = np.cos(np.pi / 2), np.sin(np.pi / 2)
    out = np.zeros((2 * len(params["limbs_point"]), h, w))
    for l, (ja, jb) in enumerate(params["limbs_point"]):
        cnt = np.zeros((h, w))
        for pose in poses:
            (fx, fy, fv), (tx, ty, tv) = pose[ja], pose[jb]
            if not (fv > 0 and tv > 0) or (fx == tx and fy == ty):
                continue
            dx, dy = tx - fx, ty - fy
            dist = np.sqrt(dx * dx + dy * dy)
            ux, uy = dx / dist, dy / dist
            vx, vy = c * ux + s * uy, -s * ux + c * uy
            hip = ux * (gx - fx) + uy * (gy - fy)
            vip = vx * (gx - fx) + vy * (gy - fy)
            flag = (0 <= hip) & (hip <= dist) & (np.abs(vip) <= paf_width)
            out[2 * l][flag] += ux
            out[2 * l + 1][flag] += uy
            cnt += flag
        nz = cnt > 0
        out[2 * l][nz] /= cnt[nz]
        out[2 * l + 1][nz] /= cnt[nz]
    return out


def dilate_np(mask):
    """cv2.MORPH_DILATE with ones((16, 16)) (anchor 8, 8; pixels outside the image ignored): a set
    pixel s sets s-7 .. s+8 on each axis.  mask (..., h, w) -> bool."""
    out = np.asarray(mask) != 0
    for axis in (-2, -1):
        src = np.moveaxis(out, axis, -1)
        dst = np.zeros_like(src)
        L = src.shape[-1]
        for k in range(-(DILATE // 2 - 1), DILATE // 2 + 1):  # destination = source + k
            lo, hi = max(0, -k), min(L, L - k)
            if lo < hi:
                dst[..., lo + k:hi + k] |= src[..., lo:hi]
        out = np.moveaxis(dst, -1, axis)
    return out


def resize_images_np(x, oh, ow):
    """F.resize_images (Chainer <= 6: align-corners bilinear, f64 weights cast to f32, then
    ((w1 x00 + w2 x01) + w3 x10) + w4 x11 in f32) on (..., h, w) f32, as the library's own resize."""
    x = np.asarray(x, np.float32)
    h, w = x.shape[-2:]

    def taps(L, oL):
        u = np.linspace(0, L - 1, oL)
        i0 = np.clip(np.floor(u), 0, L - 2).astype(np.int64)
        return i0, (i0 + 1) - u, u - i0

    v0, dv1, dv0 = taps(h, oh)
    u0, du1, du0 = taps(w, ow)
    w1 = (du1[None, :] * dv1[:, None]).astype(np.float32)
    w2 = (du0[None, :] * dv1[:, None]).astype(np.float32)
    w3 = (du1[None, :] * dv0[:, None]).astype(np.float32)
    w4 = (du0[None, :] * dv0[:, None]).astype(np.float32)
    r0, r1, c0, c1 = v0[:, None], v0[:, None] + 1, u0[None, :], u0[None, :] + 1
    y = w1 * x[..., r0, c0] + w2 * x[..., r0, c1]
    y = y + w3 * x[..., r1, c0]
    return y + w4 * x[..., r1, c1]


def make_labels_np(poses_per_frame, h, w, mask=None, downscale=8,
                   heatmap_sigma=train_params["heatmap_sigma"], paf_width=train_params["paf_sigma"]):
    """``make_labels`` on the host: the full-resolution labels in float64 cast to f32, then (for
    downscale > 1) resize_images of the targets and ``resize_images(mask) > 0``."""
    n = len(poses_per_frame)
    oh, ow = _out_size(h, w, downscale)
    pafs = np.stack([pafs_np(p, h, w, paf_width) for p in poses_per_frame]).astype(np.float32) \
        if n else np.zeros((0, _lib.N_PAF, h, w), np.float32)
    heat = np.stack([heatmaps_np(p, h, w, heatmap_sigma) for p in poses_per_frame]).astype(np.float32) \
        if n else np.zeros((0, _lib.N_HEAT, h, w), np.float32)
    ign = dilate_np(_lib.pack_mask(mask, n, h, w)) if mask is not None else np.zeros((n, h, w), bool)
    if int(downscale) == 1:
        return pafs, heat, ign
    return resize_images_np(pafs, oh, ow), resize_images_np(heat, oh, ow), \
        resize_images_np(ign.astype(np.float32), oh, ow) > 0
