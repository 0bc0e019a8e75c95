"""The fixtures of tests/golden/jpeg (tests/golden/make_golden_jpeg.py writes them), read once."""
import functools
import os

import numpy as np

from conftest import GOLDEN

DIR = os.path.join(GOLDEN, "jpeg")
NEGATIVE = {"bad_progressive.jpg": 1, "bad_truncated.jpg": 2, "bad_random.jpg": 2}  # the decode's status


@functools.lru_cache(maxsize=None)
def files():
    """{file name: bytes} of every fixture."""
    return {n: open(os.path.join(DIR, n), "rb").read() for n in sorted(os.listdir(DIR)) if n.endswith(".jpg")}


@functools.lru_cache(maxsize=None)
def pixels():
    """{file name: Pillow's (h, w, 3) uint8 BGR decode} of the decodable fixtures."""
    return dict(np.load(os.path.join(DIR, "pixels.npz")))


def positive():
    return [n for n in files() if n not in NEGATIVE]


@functools.lru_cache(maxsize=None)
def stated(name):
    """jpeg.decode_np of a fixture (the NumPy statement), computed once per session."""
    from conftest import pkg_module
    out = pkg_module("jpeg").decode_np(files()[name])
    out.setflags(write=False)
    return out


RANGE_SOURCE = "37x45_422_q90.jpg"  # noise at a fine quality: large coefficients


@functools.lru_cache(maxsize=None)
def range_file():
    """RANGE_SOURCE with every entry of its quantisation tables set to 255: still a baseline file
    Pillow decodes (to other pixels), but sum |coef q| of its blocks is far past the 32-bit inverse
    DCT's bound, so the device path turns it down with OP_JPEG_RANGE."""
    data = bytearray(files()[RANGE_SOURCE])
    at = 2
    while data[at + 1] != 0xDA:
        length = (data[at + 2] << 8) | data[at + 3]
        if data[at + 1] == 0xDB:
            for q in range(at + 4, at + 2 + length, 65):
                data[q + 1:q + 65] = b"\xff" * 64
        at += 2 + length
    return bytes(data)
