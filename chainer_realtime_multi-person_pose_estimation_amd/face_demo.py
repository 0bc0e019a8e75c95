"""camera_face_demo.py's loop body over image files: find faces with the Haar cascade
(haar.CascadeClassifier, the reference's detectMultiScale call), crop each, run FaceNet on the crop,
draw the white rectangle and the face keypoints.

  python -m chainer_realtime_multi-person_pose_estimation_amd.face_demo --cascade XML --weights facenet.npz \\
      --img A [--img B ...] [--out result.png] [--device-crops] [--staged] [--random-weights]

``crop_face`` restates camera_face_demo.py:10-24, which clips to W / H (face_detector.crop_face, the
other copy in the reference, clips to W-1 / H-1).  With ``--device-crops`` a box goes through
``FaceDetector.detect_rois`` (the crop is cut on the device) only when that crop equals the padded
square: ``device_box`` says when; the other boxes take the host crop, so the keypoints are the same
either way.  ``--staged`` stages the frames (one size), finds the faces with ``detect_staged`` and runs
FaceNet with ``detect_rois_staged``: the frames go up once.  Camera capture is not part of this.
"""
import numpy as np

from . import _lib
from . import weights as _weights
from .constants import params
from .demo import draw_rectangle
from .draw import read_bgr, write_bgr
from .face_detector import FaceDetector, draw_face_keypoints
from .haar import DEFAULTS, CascadeClassifier

WHITE = (255, 255, 255)


def crop_bounds(shape, rect):
    """camera_face_demo.py:12-19: (left, top, right, bottom) of the rect scaled by face_crop_scale about
    its centre, clipped to [0, W] x [0, H]."""
    h, w = shape[:2]
    cx, cy = rect[0] + rect[2] / 2, rect[1] + rect[3] / 2
    cw, ch = rect[2] * params["face_crop_scale"], rect[3] * params["face_crop_scale"]
    return (max(0, int(cx - cw / 2)), max(0, int(cy - ch / 2)), min(w, int(cx + cw / 2)), min(h, int(cy + ch / 2)))


def crop_face(img, rect):
    """camera_face_demo.py:10-24 -> (the crop in the top-left corner of a zero square whose side is its
    longer edge, (left, top))."""
    left, top, right, bottom = crop_bounds(img.shape, rect)
    cropped = img[top:bottom, left:right]
    side = max(cropped.shape[:-1])
    padded = np.zeros((side, side, cropped.shape[-1]), np.uint8)
    padded[:cropped.shape[0], :cropped.shape[1]] = cropped
    return padded, (left, top)


def device_box(shape, rect):
    """The (left, top, right, bottom) box whose ``face_detector.roi_crop_np`` equals ``crop_face``'s
    square, or None: along each axis the crop fills the square or ends at the frame's edge (what lies
    past the edge is zero in both)."""
    h, w = shape[:2]
    left, top, right, bottom = crop_bounds(shape, rect)
    side = max(right - left, bottom - top)
    if side < 1 or (right - left != side and right != w) or (bottom - top != side and bottom != h):
        return None
    return (left, top, left + side, top + side)


def annotate(img, rects, keypoints):
    """The reference's drawing for one frame: per face the rectangle, then its keypoints."""
    res = img.copy()
    for rect, kps in zip(rects, keypoints):
        draw_rectangle(res, (int(rect[0]), int(rect[1])), (int(rect[0] + rect[2]), int(rect[1] + rect[3])), WHITE)
        res = draw_face_keypoints(res, kps, crop_bounds(img.shape, rect)[:2])
    return res


def run(cascade, face_detector, imgs, device_crops=False, staged=False):
    """-> [(drawn image, rects (n, 4), [keypoints of face 0, ...])] per image.  ``staged`` needs frames
    of one size and implies device crops."""
    imgs = [np.ascontiguousarray(i) for i in imgs]
    ctx = None
    if staged:
        ctx = _lib.Context(cascade.device)
        ctx.stage_frames(np.stack(imgs))
        all_rects = cascade.detect_staged(ctx, 0, len(imgs), **_cv_names())
    else:
        all_rects = cascade.detect_batch(imgs, **_cv_names())
    try:
        out = []
        for f, (img, rects) in enumerate(zip(imgs, all_rects)):
            kps = [None] * len(rects)
            boxes = [device_box(img.shape, r) if (device_crops or staged) else None for r in rects]
            on_device = [i for i, b in enumerate(boxes) if b is not None]
            if on_device:
                bx = [boxes[i] for i in on_device]
                got = (face_detector.detect_rois_staged(ctx, f, 1, bx) if staged else face_detector.detect_rois(img, bx))
                for i, k in zip(on_device, got):
                    kps[i] = k
            for i, r in enumerate(rects):
                if kps[i] is None:
                    kps[i] = face_detector(crop_face(img, r)[0])
            out.append((annotate(img, rects, kps), rects, kps))
        return out
    finally:
        if ctx is not None:
            ctx.close()


def _cv_names():
    return dict(scaleFactor=DEFAULTS["scale_factor"], minNeighbors=DEFAULTS["min_neighbors"], minSize=DEFAULTS["min_size"])


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="Face detector on the faces a Haar cascade finds")
    ap.add_argument("--cascade", required=True, help="opencv-cascade-classifier XML (models/haarcascade_frontalface_alt.xml)")
    ap.add_argument("--weights", help="FaceNet weights (facenet.npz)")
    ap.add_argument("--random-weights", action="store_true", help="seeded random FaceNet weights (plumbing run)")
    ap.add_argument("--img", action="append", required=True, help="image file path (repeat for more)")
    ap.add_argument("--out", action="append", help="output image path per --img (default result.png, result_1.png, ...)")
    ap.add_argument("--gpu", "-g", type=int, default=-1, help="HIP device (negative: device 0; no CPU path)")
    ap.add_argument("--device-crops", action="store_true", help="cut the crops on the device where that gives the same crop")
    ap.add_argument("--staged", action="store_true", help="stage the frames once and read them in place (frames of one size)")
    args = ap.parse_args(argv)
    device = max(args.gpu, 0)
    outs = args.out or ["result.png" if i == 0 else "result_%d.png" % i for i in range(len(args.img))]
    if len(outs) != len(args.img):
        ap.error("as many --out as --img")
    if not args.weights and not args.random_weights:
        ap.error("--weights is required (or --random-weights)")
    model = _weights.random_weights(0, arch="facenet") if args.random_weights else None
    face_detector = FaceDetector("facenet", args.weights, model=model, device=device)
    cascade = CascadeClassifier(args.cascade, device=device)
    results = run(cascade, face_detector, [read_bgr(p) for p in args.img], args.device_crops, args.staged)
    for path, (res, rects, _) in zip(outs, results):
        print("%d face(s); saving result into %s..." % (len(rects), path))
        write_bgr(path, res)
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
