"""Whole-body detection over a staged batch: the loop of the reference's demo.py (pose, then a face
and two hands per person) at the batch sizes of the throughput path, without leaving the device.

``body_rois_np`` is the statement of the boxes: ``PoseDetector.get_unit_length``, ``face_bbox`` and
``hand_bboxes`` (pose_detector.py:267-297, 354-399 of the reference) with every operation written
out, one IEEE double operation at a time and no BLAS call.  The helpers themselves go through
``np.linalg.norm`` (BLAS ``ddot``), whose last bits depend on the BLAS build, so they agree with this
statement in the boxes and to ~1e-16 relative in ``unit``; the device kernel (csrc/body.hip,
``_lib.body_rois`` / ``Context.body_rois``) agrees with this statement bit for bit.

``detect_staged`` runs the three steps on staged frames: one ``Context.body_rois`` call (the boxes
from the result rows where they lie), one ``detect_rois_staged`` call per network (the staged
frames read in place, the ROIs in chunks of ``roi_batch``).
"""
import numpy as np

from . import _lib
from .constants import JointType, params

# pose_detector.py:278-290: the base limbs with their divisors, and every limb's divisor
UNIT_BASE = (14, 3, 0, 13, 9)
UNIT_BASE_DIV = (0.85, 2.2, 2.2, 0.85, 0.85)
UNIT_ALL_DIV = (2.2, 1.7, 1.7, 2.2, 1.7, 1.7, 0.6, 0.93, 0.65, 0.85, 0.6, 0.93, 0.65, 0.85, 1.0, 0.2, 0.2, 0.25, 0.25)

ABSENT, VALID, SKIPPED = 0, 1, 2  # the states of a box
COORD_MAX = 2 ** 30               # op_cpm_detect_rois: no coordinate beyond +-2^30
AREA_MAX = 2 ** 31                # ... and (r-l) * (b-t) below 2^31
PARTS = ("face", "left", "right")


def pairwise_sum(terms):
    """``np.sum`` of up to 128 contiguous doubles, addition by addition (NumPy's pairwise_sum below
    its block size): sequential for fewer than 8 terms, else eight accumulators seeded with terms
    0..7, full blocks of 8 added lane-wise, ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the tail."""
    q = [np.float64(v) for v in terms]
    n = len(q)
    if n < 8:
        s = np.float64(0.0)
        for v in q:
            s = s + v
        return s
    r = q[:8]
    i = 8
    while i < n - n % 8:
        for j in range(8):
            r[j] = r[j] + q[i + j]
        i += 8
    s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    while i < n:
        s = s + q[i]
        i += 1
    return s


def _box(present, l, t, r, b):
    """-> ((l, t, r, b) ints, state): truncated toward zero; SKIPPED and zeros for a box
    op_cpm_detect_rois would refuse (not finite, beyond +-2^30, thinner than 2, area >= 2^31)."""
    if not present:
        return (0, 0, 0, 0), ABSENT
    v = [np.trunc(x) for x in (l, t, r, b)]
    if not all(-COORD_MAX <= x <= COORD_MAX for x in v):  # false for NaN and the infinities
        return (0, 0, 0, 0), SKIPPED
    l, t, r, b = (int(x) for x in v)
    if r - l < 2 or b - t < 2 or (r - l) * (b - t) >= AREA_MAX:
        return (0, 0, 0, 0), SKIPPED
    return (l, t, r, b), VALID


def body_rois_np(poses):
    """poses (P, 18, 3) f64 -> (unit (P,) f64, box (P, 3, 4) int32, state (P, 3) int32).

    Per person: ``len[i] = sqrt(dx*dx + dy*dy)`` for all 19 limbs of ``params["limbs_point"]``
    (an absent joint sits at (0, 0) and still yields a length: the reference's behaviour on pose
    rows); ``unit`` = the mean of ``len / divisor`` over the found (``len > 0``) base limbs, or over
    every found limb when no base limb was found, summed by ``pairwise_sum`` (NaN, ``np.nan``'s
    bits, when no limb was found at all); box 0 the face (nose -+ unit, 1.2 units above to 0.8
    below), boxes 1 / 2 the left / right hand (the hand, moved 0.3 of elbow -> hand when the elbow
    was found, -+ 0.95 unit), each truncated toward zero.  ``poses`` is not modified: the
    reference's in-place shift of the hand joints stays local.  state: ABSENT, VALID or SKIPPED."""
    poses = np.asarray(poses, np.float64).reshape(-1, len(JointType), 3)
    n = len(poses)
    unit = np.zeros(n, np.float64)
    box = np.zeros((n, 3, 4), np.int32)
    state = np.zeros((n, 3), np.int32)
    limbs = [(int(a), int(b)) for a, b in params["limbs_point"]]
    with np.errstate(all="ignore"):
        for p, pose in enumerate(poses):
            length = []
            for a, b in limbs:
                dx, dy = pose[b][0] - pose[a][0], pose[b][1] - pose[a][1]
                length.append(np.sqrt(dx * dx + dy * dy))
            if any(length[i] > 0 for i in UNIT_BASE):
                terms = [length[i] / np.float64(d) for i, d in zip(UNIT_BASE, UNIT_BASE_DIV) if length[i] > 0]
            else:
                terms = [v / np.float64(d) for v, d in zip(length, UNIT_ALL_DIV) if v > 0]
            u = pairwise_sum(terms) / np.float64(len(terms)) if terms else np.float64(np.nan)
            unit[p] = u
            nx, ny, nv = pose[JointType.Nose]
            boxes = [_box(nv > 0, nx - u, ny - u * 1.2, nx + u, ny + u * 0.8)]
            s = u * 0.95
            for hand, elbow in ((JointType.LeftHand, JointType.LeftElbow), (JointType.RightHand, JointType.RightElbow)):
                x, y, v = pose[hand]
                if pose[elbow][2] > 0:
                    x = x + 0.3 * (x - pose[elbow][0])
                    y = y + 0.3 * (y - pose[elbow][1])
                boxes.append(_box(v > 0, x - s, y - s, x + s, y + s))
            for k, (bx, st) in enumerate(boxes):
                box[p, k] = bx
                state[p, k] = st
    return unit, box, state


def detect_staged(pose_detector, face_detector, hand_detector, first, n, roi_batch=128, cap=64):
    """Poses, faces and hands of staged frames [first, first + n) of ``pose_detector``'s context,
    after its staged run (``PoseDetector.run_staged``): a list with, per frame, the list of its persons

        {"pose": (18, 3) f64, "score": float, "unit": float, "skipped": (parts...),
         "face": (keypoints, bbox) or None, "hands": {"left": (keypoints, bbox) or None, "right": ...}}

    One ``Context.body_rois`` call makes every box on the device; one ``detect_rois_staged`` call
    per network reads the staged frames in place.  The ROIs go in ``demo.run``'s order: the faces
    frame by frame and person by person; the hands alike, left then right per person.  A frame over
    the batched post-process caps (``frame_status`` OP_ERR_CAPACITY) or with more than ``cap``
    persons is taken through ``fetch_result`` and ``_lib.body_rois``; its ROIs join the same calls.
    A box the ROI detector cannot run (state SKIPPED: not finite, thinner than 2 px, ...) comes back
    as ``(None, None)`` with its part named in ``"skipped"``; ``demo.run`` would have raised there.

    ``roi_batch``: ROIs per forward.  It is a memory bound -- the largest split activation of one
    368 x 368 ROI is about 35 MB -- not a tuned number: nobody has measured other values."""
    ctx = pose_detector.staged_context()
    first, n = int(first), int(n)
    count, status, unit, box, state = ctx.body_rois(first, n, cap)
    results = ctx.fetch_results(first, n, cap=cap)
    frames = []
    for i in range(n):
        poses, scores, _ = results[i]
        u, bx, st = unit[i], box[i], state[i]
        if status[i] == _lib.OP_ERR_CAPACITY or count[i] > cap:
            poses, scores, _ = ctx.fetch_result(first + i, cap=max(int(count[i]), cap))
            u, bx, st = _lib.body_rois(poses, device=pose_detector.device)
        if len(poses) > len(u):
            raise RuntimeError("wholebody.detect_staged: frame %d has %d persons and %d box rows" % (first + i, len(poses), len(u)))
        frames.append([{"pose": poses[p], "score": float(scores[p]), "unit": float(u[p]), "face": None,
                        "hands": {"left": None, "right": None}, "skipped": (),
                        "_box": np.asarray(bx[p]), "_state": np.asarray(st[p])} for p in range(len(poses))])
    # the ROI lists, in demo.run's order
    face_rois, hand_rois = [], []
    for i, persons in enumerate(frames):
        for person in persons:
            if person["_state"][0] == VALID:
                face_rois.append((i, person, tuple(int(v) for v in person["_box"][0])))
            for k, side in ((1, "left"), (2, "right")):
                if person["_state"][k] == VALID:
                    hand_rois.append((i, person, tuple(int(v) for v in person["_box"][k]), side))
    if face_rois:
        face_detector.set_roi_batch(roi_batch)
        kps = face_detector.detect_rois_staged(ctx, first, n, [r[2] for r in face_rois], [r[0] for r in face_rois])
        for (_, person, bbox), kp in zip(face_rois, kps):
            person["face"] = (kp, bbox)
    if hand_rois:
        hand_detector.set_roi_batch(roi_batch)
        kps = hand_detector.detect_rois_staged(ctx, first, n, [r[2] for r in hand_rois], [r[3] for r in hand_rois],
                                               [r[0] for r in hand_rois])
        for (_, person, bbox, side), kp in zip(hand_rois, kps):
            person["hands"][side] = (kp, bbox)
    for persons in frames:
        for person in persons:
            st = person.pop("_state")
            person.pop("_box")
            person["skipped"] = tuple(name for k, name in enumerate(PARTS) if st[k] == SKIPPED)
            if st[0] == SKIPPED:
                person["face"] = (None, None)
            for k, side in ((1, "left"), (2, "right")):
                if st[k] == SKIPPED:
                    person["hands"][side] = (None, None)
    return frames
