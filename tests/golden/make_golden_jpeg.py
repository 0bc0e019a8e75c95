"""Writes tests/golden/jpeg/: small baseline JPEG files encoded with Pillow (libjpeg-turbo) from crops
of people.png and from seeded noise, three files outside the decodable subset, and pixels.npz with
Pillow's own decode of every decodable file (BGR), keyed by file name.

    python tests/golden/make_golden_jpeg.py

The grid is the smallest set of cases in which each rule of the decode can go wrong: sizes around
the block and MCU sizes and the narrow-plane threshold of the chroma filters, every sampling the
device path takes, a coarse and a fine quality, optimised Huffman tables and restart intervals.
"""
import io
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "jpeg")
SIZES = [(1, 1), (9, 4), (9, 5), (8, 8), (16, 16), (17, 33), (37, 45), (40, 56)]
SAMPLING = [("grey", None), ("444", 0), ("422", 1), ("420", 2)]
QUALITY = [20, 90]


def encode(rgb, sampling, **kw):
    buf = io.BytesIO()
    if sampling is None:
        Image.fromarray(rgb).convert("L").save(buf, "JPEG", **kw)
    else:
        Image.fromarray(rgb).save(buf, "JPEG", subsampling=sampling, **kw)
    return buf.getvalue()


def pillow_bgr(data):
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[:, :, ::-1])


def main():
    os.makedirs(OUT, exist_ok=True)
    photo = np.asarray(Image.open(os.path.join(HERE, "people.png")).convert("RGB"))
    rng = np.random.default_rng(2017)
    files = {}
    k = 0
    for h, w in SIZES:
        for name, sampling in SAMPLING:
            for q in QUALITY:
                if (k // 2 + k) % 2:
                    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
                else:
                    y0, x0 = 40 + 5 * k, 30 + 6 * k
                    rgb = np.ascontiguousarray(photo[y0:y0 + h, x0:x0 + w])
                assert rgb.shape == (h, w, 3)
                files["%dx%d_%s_q%d.jpg" % (h, w, name, q)] = encode(rgb, sampling, quality=q)
                k += 1
    crop = np.ascontiguousarray(photo[100:137, 200:245])  # 37 x 45
    files["37x45_420_q75_optimize.jpg"] = encode(crop, 2, quality=75, optimize=True)
    files["37x45_420_q75_restart_blocks2.jpg"] = encode(crop, 2, quality=75, restart_marker_blocks=2)
    files["37x45_422_q75_restart_rows1.jpg"] = encode(crop, 1, quality=75, restart_marker_rows=1)
    pixels = {name: pillow_bgr(data) for name, data in files.items()}
    # outside the subset
    files["bad_progressive.jpg"] = encode(crop, 2, quality=75, progressive=True)
    whole = encode(np.ascontiguousarray(photo[100:140, 200:256]), 2, quality=75)
    files["bad_truncated.jpg"] = whole[:len(whole) - 120]  # cut in the middle of the scan
    files["bad_random.jpg"] = b"\xff\xd8" + rng.integers(0, 256, 40, dtype=np.uint8).tobytes()
    for name, data in files.items():
        with open(os.path.join(OUT, name), "wb") as f:
            f.write(data)
    np.savez_compressed(os.path.join(OUT, "pixels.npz"), **pixels)
    total = sum(len(d) for d in files.values()) + os.path.getsize(os.path.join(OUT, "pixels.npz"))
    print("%d files, %d bytes with pixels.npz" % (len(files), total))


if __name__ == "__main__":
    main()
