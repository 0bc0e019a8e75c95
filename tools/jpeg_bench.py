"""Timing of the device JPEG path next to the path it replaces, on frames a user would
run: people.png resized and tiled to 640 x 480 and to 1280 x 720, encoded by Pillow at quality 90 in
4:2:0, 232 distinct frames (each shifted by a few pixels) written to a temporary directory.

    python tools/jpeg_bench.py [--frames 232] [--repeats 5] [--sizes 480x640,720x1280]

Per size, after one warm-up of each path, the median of --repeats runs of
  (a) the parent path: draw.read_bgr (Pillow, one host thread) per file into one array, then
      Context.stage_frames -- host wall time, ending in the call's own synchronise;
  (b) reading the files' bytes and Context.stage_jpegs (op_jpeg_stage) -- host wall time, the call
      returns once the frames are staged;
  (c) op_jpeg_last_ms of (b)'s call at 1, 4 and 16 entropy-decode threads: the host's entropy-decode
      wall time and the device time (stream events around the uploads and the two kernels);
  (d) the bytes the two kernels must move (coefficients in, planes out and in again, BGR out) over
      that device time, as a fraction of the HBM bandwidth a copy kernel reaches (6.29 TB/s); the
      device time includes the coefficient upload, which the figure therefore charges to the kernels.
The staged frames are compared with Pillow's pixels once per size.  One JSON line at the end.  Needs
the device: there is no other path."""
import argparse
import importlib
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PKG = "chainer_realtime_multi-person_pose_estimation_amd"
HBM_COPY_BYTES_PER_S = 6.29e12


def make_files(root, h, w, n):
    from PIL import Image
    src = Image.open(os.path.join(REPO, "tests", "golden", "people.png")).convert("RGB")
    side = max(h, (w + 1) // 2)
    tile = np.asarray(src.resize((side, side), Image.BILINEAR))
    base = np.tile(tile, (1, 2, 1))[:h, :w]
    paths = []
    for k in range(n):
        p = os.path.join(root, "%dx%d_%04d.jpg" % (h, w, k))
        Image.fromarray(np.ascontiguousarray(np.roll(base, (3 * k, 5 * k), axis=(0, 1)))).save(p, quality=90, subsampling=2)
        paths.append(p)
    return paths


def median_of(fn, repeats):
    fn()  # warm-up
    out = []
    for _ in range(repeats):
        out.append(fn())
    if isinstance(out[0], tuple):
        return tuple(statistics.median(v[i] for v in out) for i in range(len(out[0])))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=232)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="480x640,720x1280")
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats must be at least 5")
    L = importlib.import_module(PKG + "._lib")
    draw = importlib.import_module(PKG + ".draw")
    render = importlib.import_module(PKG + ".render")
    ctx = L.Context(0)
    result = {"frames": args.frames, "repeats": args.repeats, "quality": 90, "sampling": "4:2:0", "sizes": {}}
    with tempfile.TemporaryDirectory() as root:
        for size in args.sizes.split(","):
            h, w = (int(v) for v in size.split("x"))
            paths = make_files(root, h, w, args.frames)
            n = len(paths)

            def parent():
                t0 = time.perf_counter()
                frames = np.empty((n, h, w, 3), np.uint8)
                for k, p in enumerate(paths):
                    frames[k] = draw.read_bgr(p)
                ctx.stage_frames(frames)
                return (time.perf_counter() - t0) * 1e3

            def device():
                t0 = time.perf_counter()
                datas = []
                for p in paths:
                    with open(p, "rb") as f:
                        datas.append(f.read())
                status = ctx.stage_jpegs(datas, h, w)
                ms = (time.perf_counter() - t0) * 1e3
                assert not status.any(), status
                return (ms,) + L.jpeg_last_ms(0)

            r = {"file_bytes": sum(os.path.getsize(p) for p in paths)}
            r["parent_read_bgr_stage_frames_ms"] = median_of(parent, args.repeats)
            for threads in (1, 4, 16):
                L.jpeg_set_threads(threads)
                wall, host_ms, dev_ms = median_of(device, args.repeats)
                r["threads_%d" % threads] = {"stage_jpegs_wall_ms": wall, "entropy_decode_ms": host_ms, "device_ms": dev_ms}
            assert np.array_equal(render.render_staged(ctx, n - 1, 1, [[]])[0], draw.read_bgr(paths[-1]))
            info = L.jpeg_probe(open(paths[0], "rb").read())
            blocks = int(info.n_blocks) * n
            moved = blocks * 128 + 2 * blocks * 64 + n * h * w * 3
            r["kernel_bytes"] = moved
            r["hbm_fraction_of_device_time"] = moved / (r["threads_16"]["device_ms"] * 1e-3) / HBM_COPY_BYTES_PER_S
            r["frames_per_s_parent"] = n / (r["parent_read_bgr_stage_frames_ms"] * 1e-3)
            r["frames_per_s_stage_jpegs_16"] = n / (r["threads_16"]["stage_jpegs_wall_ms"] * 1e-3)
            result["sizes"][size] = r
            print("%s: parent %.1f ms, stage_jpegs %.1f ms at 16 threads (entropy %.1f ms, device %.1f ms)" % (
                size, r["parent_read_bgr_stage_frames_ms"], r["threads_16"]["stage_jpegs_wall_ms"],
                r["threads_16"]["entropy_decode_ms"], r["threads_16"]["device_ms"]), file=sys.stderr)
    ctx.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
