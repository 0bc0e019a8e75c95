"""demo.py of the reference (demo.py:1-60): pose, then per person the face and both hands.

    python -m chainer_realtime_multi-person_pose_estimation_amd.demo --img IMG [--gpu G]

Loads models/coco_posenet.npz, models/handnet.npz and models/facenet.npz (the reference's fixed
paths; ``--models DIR`` changes the directory, ``--random-weights`` uses seeded random weights for
a plumbing run without trained weights), runs PoseDetector on the image, blends the skeletons in
(``cv2.addWeighted(img, 0.6, pose, 0.4, 0)``), then for every person crops the face and the hands
(PoseDetector.get_unit_length / crop_face / crop_hands), runs FaceDetector / HandDetector on the
crops and draws their keypoints and white crop rectangles; writes result.png.

``--img`` may be given several times; ``--staged`` takes the images (all of one size) through the
staged batch instead (``run_batch``: one staged pose step, ``wholebody.detect_staged``, one device
draw) and writes result.png for one image, result_<k>.png for several.
"""
import argparse
import os
import sys

import numpy as np

from . import weights as _weights
from .draw import draw_line, draw_person_pose, read_bgr, write_bgr
from .face_detector import FaceDetector, draw_face_keypoints
from .hand_detector import HandDetector, draw_hand_keypoints
from .pose_detector import PoseDetector


def add_weighted(a, wa, b, wb, gamma=0.0):
    """cv2.addWeighted on uint8: saturate(round(a*wa + b*wb + gamma))."""
    v = a.astype(np.float64) * wa + b.astype(np.float64) * wb + gamma
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def draw_rectangle(img, p0, p1, color):
    """cv2.rectangle(img, p0, p1, color, 1): the four 1-px edges."""
    (x0, y0), (x1, y1) = p0, p1
    for a, b in (((x0, y0), (x1, y0)), ((x1, y0), (x1, y1)), ((x1, y1), (x0, y1)), ((x0, y1), (x0, y0))):
        draw_line(img, a, b, color, 1)


def run(img, pose_detector, face_detector, hand_detector, log=print, device_draw=False, device_crops=False):
    """demo.py:20-56.  The crops of every person are detected in two batched forwards (faces,
    hands: ``detect_batch``) and drawn in the reference's per-person order, so the image is the
    same as with one detector call per crop.  ``device_draw``: the same drawing as one display
    list in one device call (render.demo_list, render.render); the image is the same bit for bit.
    ``device_crops``: the detectors get the image and the boxes (PoseDetector.face_bbox /
    hand_bboxes, one ``detect_rois`` call each) and cut, mirror and resize the crops on the
    device; the keypoints, and so the image, are the same bit for bit."""
    log("Estimating pose...")
    person_pose_array, _ = pose_detector(img)
    if device_draw:  # the poses as they are drawn: crop_hands below shifts the hand joints in place
        drawn_poses = np.array(person_pose_array, copy=True)
    else:
        res_img = add_weighted(img, 0.6, draw_person_pose(img, person_pose_array), 0.4, 0)
    faces, hands = [], []
    if device_crops:
        # boxes only: (True, bbox) / {"bbox": bbox} stand where the default path holds the crops
        for person_pose in person_pose_array:
            unit_length = pose_detector.get_unit_length(person_pose)
            bbox = pose_detector.face_bbox(person_pose, unit_length)
            faces.append((None, None) if bbox is None else (True, bbox))
            boxes = pose_detector.hand_bboxes(person_pose, unit_length)
            hands.append({side: None if boxes[side] is None else {"bbox": boxes[side]} for side in ("left", "right")})
        face_boxes = [f[1] for f in faces if f[0] is not None]
        hand_boxes = [(h[side]["bbox"], side) for h in hands for side in ("left", "right") if h[side] is not None]
        face_kps = iter(face_detector.detect_rois(img, face_boxes) if face_boxes else [])
        hand_kps = iter(hand_detector.detect_rois(img, [b for b, _ in hand_boxes], [s for _, s in hand_boxes])
                        if hand_boxes else [])
    else:
        for person_pose in person_pose_array:
            unit_length = pose_detector.get_unit_length(person_pose)
            faces.append(pose_detector.crop_face(img, person_pose, unit_length))
            hands.append(pose_detector.crop_hands(img, person_pose, unit_length))
        face_crops = [f[0] for f in faces if f[0] is not None]
        hand_crops = [(h[side]["img"], side) for h in hands for side in ("left", "right") if h[side] is not None]
        face_kps = iter(face_detector.detect_batch(face_crops) if face_crops else [])
        hand_kps = iter(hand_detector.detect_batch([c for c, _ in hand_crops], [s for _, s in hand_crops])
                        if hand_crops else [])
    if device_draw:
        from . import render
        face_items, hand_items = [], []
        for (cropped_face_img, bbox), person_hands in zip(faces, hands):
            log("Estimating face keypoints...")
            face_items.append((next(face_kps), bbox) if cropped_face_img is not None else None)
            log("Estimating hands keypoints...")
            hand_items.append({side: (next(hand_kps), person_hands[side]["bbox"]) if person_hands[side] is not None
                               else None for side in ("left", "right")})
        prims = render.demo_list(drawn_poses, face_items, hand_items)
        return render.render([img], [prims], device=pose_detector.device)[0]
    for (cropped_face_img, bbox), person_hands in zip(faces, hands):
        log("Estimating face keypoints...")
        if cropped_face_img is not None:
            res_img = draw_face_keypoints(res_img, next(face_kps), (bbox[0], bbox[1]))
            draw_rectangle(res_img, (bbox[0], bbox[1]), (bbox[2], bbox[3]), (255, 255, 255))
        log("Estimating hands keypoints...")
        for side in ("left", "right"):
            if person_hands[side] is not None:
                bbox = person_hands[side]["bbox"]
                res_img = draw_hand_keypoints(res_img, next(hand_kps), (bbox[0], bbox[1]))
                draw_rectangle(res_img, (bbox[0], bbox[1]), (bbox[2], bbox[3]), (255, 255, 255))
    return res_img


def run_batch(frames, pose_detector, face_detector, hand_detector, log=print, device_draw=True, roi_batch=128):
    """``run`` for a batch of equally sized frames without leaving the device between the steps:
    the frames are staged once, the pose step runs on all of them (``PoseDetector.run_staged``),
    ``wholebody.detect_staged`` makes the boxes on the device from the poses where they lie and runs
    FaceNet / HandNet on the staged frames in place, and every frame's drawing (``render.demo_list``)
    is painted in one ``render.render_staged`` call (``device_draw=False``: ``render.render_np`` per
    frame, the same pixels).  -> the list of result images.  A box the ROI detector cannot run is
    left out of the drawing (``run`` would raise there)."""
    from . import render, wholebody
    frames = np.ascontiguousarray(np.stack([np.asarray(f) for f in frames]))
    log("Estimating pose...")
    n = pose_detector.run_staged(frames)
    log("Estimating face and hands keypoints...")
    result = wholebody.detect_staged(pose_detector, face_detector, hand_detector, 0, n, roi_batch=roi_batch)
    drawn = lambda item: item if item is not None and item[0] is not None else None  # skipped boxes are not drawn
    lists = []
    for persons in result:
        poses = np.array([p["pose"] for p in persons]).reshape(-1, 18, 3)
        lists.append(render.demo_list(poses, [drawn(p["face"]) for p in persons],
                                      [{side: drawn(p["hands"][side]) for side in ("left", "right")} for p in persons]))
    if device_draw:
        return list(render.render_staged(pose_detector.staged_context(), 0, n, lists))
    return [render.render_np(f, l) for f, l in zip(frames, lists)]


def main(argv=None):
    ap = argparse.ArgumentParser(description="Pose detector")
    ap.add_argument("--img", action="append", help="image file path (may be given several times)")
    ap.add_argument("--gpu", "-g", type=int, default=-1, help="HIP device (negative: device 0; no CPU path)")
    ap.add_argument("--models", default="models", help="directory of coco_posenet.npz / handnet.npz / facenet.npz")
    ap.add_argument("--random-weights", action="store_true", help="seeded random weights (plumbing run)")
    ap.add_argument("--out", default="result.png")
    ap.add_argument("--device-draw", action="store_true", help="draw on the device (one display list, one launch)")
    ap.add_argument("--device-crops", action="store_true",
                    help="cut the face / hand crops on the device from the image and the boxes (detect_rois)")
    ap.add_argument("--staged", action="store_true",
                    help="the staged batch: poses, boxes, face / hand keypoints and drawing without leaving the device")
    args = ap.parse_args(argv)
    if not args.img:
        ap.error("--img is required")
    pose_kw = {"max_batch": len(args.img)} if args.staged else {}
    if args.random_weights:
        pd = PoseDetector("posenet", model=_weights.random_weights(0), device=args.gpu, **pose_kw)
        hd = HandDetector("handnet", model=_weights.random_weights(0, arch="handnet"), device=args.gpu)
        fd = FaceDetector("facenet", model=_weights.random_weights(0, arch="facenet"), device=args.gpu)
    else:
        pd = PoseDetector("posenet", os.path.join(args.models, "coco_posenet.npz"), device=args.gpu, **pose_kw)
        hd = HandDetector("handnet", os.path.join(args.models, "handnet.npz"), device=args.gpu)
        fd = FaceDetector("facenet", os.path.join(args.models, "facenet.npz"), device=args.gpu)
    imgs = [read_bgr(path) for path in args.img]
    if args.staged:
        if len({im.shape for im in imgs}) != 1:
            ap.error("--staged needs images of one size")
        res_imgs = run_batch(imgs, pd, fd, hd)
    else:
        res_imgs = [run(img, pd, fd, hd, device_draw=args.device_draw, device_crops=args.device_crops) for img in imgs]
    stem, ext = os.path.splitext(args.out)
    for k, res_img in enumerate(res_imgs):
        out = args.out if len(res_imgs) == 1 else "%s_%d%s" % (stem, k, ext)
        print("Saving result into %s..." % out)
        write_bgr(out, res_img)
    return 0


if __name__ == "__main__":
    sys.exit(main())
