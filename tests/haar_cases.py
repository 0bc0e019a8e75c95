"""Frames and cascades shared by the Haar tests (test_haar_host.py, test_gpu_haar.py): every frame
comes from tests/golden/person.png or seeded noise, every statement result is computed once."""
import functools
import os

import numpy as np

from conftest import GOLDEN, pkg_module

DIR = os.path.join(GOLDEN, "haar")
REAL_XML = os.path.join(DIR, "haarcascade_frontalface_alt.xml.gz")  # the reference's file, gzip -9 -n
TINY_XML = os.path.join(DIR, "tiny_cascade.xml")
REFUSED = ("refuse_tilted.xml", "refuse_tree.xml", "refuse_lbp.xml", "refuse_hog.xml", "refuse_old_format.xml",
           "refuse_window.xml", "refuse_rect_outside.xml")
FACE = (334, 33, 114)  # x, y, side of the patch of person.png around the face


def haar():
    return pkg_module("haar")


@functools.lru_cache(None)
def real():
    return haar().load_cascade(REAL_XML)


@functools.lru_cache(None)
def tiny():
    return haar().load_cascade(TINY_XML)


@functools.lru_cache(None)
def person():
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(os.path.join(GOLDEN, "person.png")).convert("RGB"))[:, :, ::-1])


@functools.lru_cache(None)
def patch(side):
    """The face patch of person.png as grey, reduced to side x side by the statement's own resize."""
    x, y, s = FACE
    return haar().resize_np(np.ascontiguousarray(haar().grey_np(person())[y:y + s, x:x + s]), side, side)


def noise(h, w, seed=0, flat=None, pad=0):
    """BGR noise, optionally with a constant patch (y, x, h, w) and as a view with `pad` extra pixels per row."""
    img = np.random.default_rng(seed).integers(0, 256, (h, w + pad, 3), dtype=np.uint8)
    if flat:
        y, x, fh, fw = flat
        img[y:y + fh, x:x + fw] = 77
    return img[:, :w] if pad else img


def tiny_frame(pad=0):
    """61 x 45 (w x h) noise with a constant patch: every map value occurs with the tiny cascade."""
    return noise(45, 61, 0, flat=(10, 30, 12, 14), pad=pad)


@functools.lru_cache(None)
def person_candidates():
    return haar().candidates_np(person(), real())


def staged_frames():
    """Four 96 x 96 BGR crops of person.png around the face."""
    p = person()
    return np.stack([p[y:y + 96, x:x + 96] for x, y in ((340, 40), (344, 44), (330, 36), (350, 30))])


def batch():
    """The small frames of the mixed batch: 96 x 96 and 64 x 64 face patches (grey), 61 x 45 BGR noise, a
    constant frame, a 19 x 30 frame, a 20 x 20 frame, a grey crop that is not square."""
    grey = patch(96)
    return [grey, patch(64), noise(45, 61, 1), np.full((40, 50, 3), 128, np.uint8), noise(30, 19, 2),
            np.ascontiguousarray(person()[40:60, 350:370]), np.ascontiguousarray(grey[10:80, 5:90])]


@functools.lru_cache(None)
def batch_candidates(scale_factor=1.2, min_size=(1, 1), max_size=None):
    """The statement's candidates of every frame of batch(), computed once per pyramid."""
    return tuple(haar().candidates_np(f, real(), scale_factor, min_size, max_size) for f in batch())
