"""gen_ignore_mask.py of the reference on the device: the ``ignore_mask_*2017`` PNG tree from a COCO
``person_keypoints_*.json``, without pycocotools or cv2.

    python -m chainer_realtime_multi-person_pose_estimation_amd.gen_ignore_mask \\
        --annotations annotations/person_keypoints_train2017.json --out ignore_mask_train2017

Every image of the file, ids sorted, all categories (gen_ignore_mask.py:17-18), with all of its
annotations in file order (``getAnnIds(imgIds=[id])``); the image size comes from the JSON's
``images[*].height / width`` (the reference decodes the image for its shape only).  ``gen_masks``
runs on the device for ``--batch`` images per call (masks.ignore_masks), and ``{id:012d}.png``
(8-bit, 0 / 255) is written only where mask_miss has a set pixel (:113-116).

    python -m chainer_realtime_multi-person_pose_estimation_amd.gen_ignore_mask \\
        --annotations annotations/person_keypoints_val2017.json --vis --images val2017 --out vis_val2017

``--vis`` (:103-111) writes, for every image, the panel ``{id:012d}.png``: the annotation masks tinted
onto the frame with the keypoints marked, beside the mask_miss tint (maskview.panels, on the device,
``--batch`` images per call) and, as in the reference, no mask files.  The frames are read with
``draw.read_bgr`` from ``--images``/``images[*].file_name``; a frame whose decoded size differs from the
JSON's is an error.  No window is opened and no key is read: there is no cv2 here.
"""
import argparse
import json
import os
import sys

import numpy as np

from . import masks as _masks


def load_images(path, with_names=False):
    """[(image id, h, w, annotations)] of a COCO annotation file, ids sorted; ``with_names`` appends
    the image's ``file_name``."""
    with open(path) as f:
        data = json.load(f)
    anns = {}
    for ann in data.get("annotations", []):
        anns.setdefault(ann["image_id"], []).append(ann)
    return [(im["id"], int(im["height"]), int(im["width"]), anns.get(im["id"], [])) +
            ((im["file_name"],) if with_names else ())
            for im in sorted(data["images"], key=lambda im: im["id"])]


def write_png(path, mask):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(mask).astype(np.uint8) * 255).save(path)


def write_panels(args):
    """--vis: the panel of every image (at most --limit of them) into --out."""
    from . import maskview
    from .draw import read_bgr, write_bgr
    images = load_images(args.annotations, with_names=True)
    if args.limit is not None:
        images = images[:args.limit]
    os.makedirs(args.out, exist_ok=True)
    for start in range(0, len(images), args.batch):
        chunk = images[start:start + args.batch]
        samples = []
        for img_id, h, w, anns, name in chunk:
            img = read_bgr(os.path.join(args.images, name))
            if img.shape[:2] != (h, w):
                raise ValueError("image %r: %s decodes to %d x %d, the annotation file says %d x %d" % (
                    img_id, name, img.shape[0], img.shape[1], h, w))
            samples.append((img, anns))
        for (img_id, _, _, _, _), panel in zip(chunk, maskview.panels(samples, max(args.gpu, 0))):
            write_bgr(os.path.join(args.out, "{:012d}.png".format(img_id)), panel)
    print("%d images, %d panels written to %s" % (len(images), len(images), args.out))
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(description="Ignore masks of a COCO keypoints file (MI355X)")
    ap.add_argument("--annotations", required=True, help="person_keypoints_{train,val}2017.json")
    ap.add_argument("--out", required=True, help="directory of the <image id>.png files")
    ap.add_argument("--batch", type=int, default=32, help="images per device call")
    ap.add_argument("--gpu", type=int, default=0, help="HIP device")
    ap.add_argument("--vis", action="store_true", help="write the annotation / mask_miss panels instead of the masks")
    ap.add_argument("--images", help="--vis: directory of the images (images[*].file_name)")
    ap.add_argument("--limit", type=int, default=None, help="--vis: only the first N images")
    args = ap.parse_args(argv)
    if args.batch < 1:
        ap.error("--batch must be positive")
    if args.vis and not args.images:
        ap.error("--vis needs --images")
    if args.limit is not None and args.limit < 0:
        ap.error("--limit must not be negative")
    if args.vis:
        return write_panels(args)
    images = load_images(args.annotations)
    os.makedirs(args.out, exist_ok=True)
    written = 0
    for start in range(0, len(images), args.batch):
        chunk = images[start:start + args.batch]
        made = _masks.ignore_masks([(h, w, anns) for _, h, w, anns in chunk], max(args.gpu, 0))
        for (img_id, _, _, _), (_, mask_miss) in zip(chunk, made):
            if np.any(mask_miss):
                write_png(os.path.join(args.out, "{:012d}.png".format(img_id)), mask_miss)
                written += 1
    print("%d images, %d masks written to %s" % (len(images), written, args.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
