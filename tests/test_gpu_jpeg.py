"""Baseline JPEG decode on the device (csrc/jpeg.hip) against jpeg.decode_np and Pillow's own
pixels: the one-shot batch call, the staged path (the kernels write into the staged set), the
detector's run_staged_jpegs with its Pillow route, and eval_coco --device-jpeg."""
import ctypes
import json
import math

import numpy as np
import pytest

import jpeg_cases as cases
import keypoint_cases
from conftest import pkg_module

pytestmark = pytest.mark.gpu


def test_last_ms_before_and_after_the_first_call(lib):
    """Runs first of this module, the only one of the suite that decodes on device 0: no call has
    completed there yet (OP_ERR_STATE, values untouched); after one, two finite times >= 0."""
    ms = (ctypes.c_double * 2)(-1.0, -1.0)
    assert lib.lib().op_jpeg_last_ms(0, ms) == lib.OP_ERR_STATE
    assert lib.last_error() == "op_jpeg_last_ms: no op_jpeg_decode or op_jpeg_stage has completed on device 0"
    assert list(ms) == [-1.0, -1.0]
    J = pkg_module("jpeg")
    frames, status = J.decode([cases.files()["16x16_420_q20.jpg"]])
    assert status == [0] and np.array_equal(frames[0], cases.pixels()["16x16_420_q20.jpg"])
    host_ms, dev_ms = lib.jpeg_last_ms(0)
    assert math.isfinite(host_ms) and math.isfinite(dev_ms) and host_ms >= 0.0 and dev_ms > 0.0


def test_every_fixture_in_one_call():
    """All 67 decodable fixtures (8 sizes from 1 x 1 to 40 x 56, grey / 4:4:4 / 4:2:2 / 4:2:0, two
    qualities, optimised tables, restart intervals) in one op_jpeg_decode: bit for bit the statement
    and Pillow."""
    J = pkg_module("jpeg")
    names = cases.positive()
    frames, status = J.decode([cases.files()[n] for n in names])
    assert status == [0] * len(names)
    for name, got in zip(names, frames):
        want = cases.pixels()[name]
        assert got.shape == want.shape and np.array_equal(got, cases.stated(name)), name
        assert np.array_equal(got, want), name


@pytest.mark.parametrize("threads", [1, 5])
def test_failed_frames_leave_their_buffers(lib, threads):
    """Three good frames with the progressive and the truncated file between them and a file whose
    blocks are past the inverse DCT's range bound (OP_JPEG_RANGE as a frame's status): the statuses,
    the good frames right, the failed frames' buffers still holding the fill."""
    J = pkg_module("jpeg")
    names = ["37x45_420_q20.jpg", "bad_progressive.jpg", "9x5_422_q90.jpg", "bad_truncated.jpg", "17x33_grey_q20.jpg",
             "range"]
    datas = [cases.range_file() if n == "range" else cases.files()[n] for n in names]
    outs = []
    for n in names:
        shape = cases.pixels()[n].shape if n in cases.pixels() else (40, 56, 3)
        outs.append(np.full(shape, 0xA5, np.uint8))
    lib.jpeg_set_threads(threads)
    try:
        status = lib.jpeg_decode(datas, outs)
    finally:
        lib.jpeg_set_threads(0)  # the default again
    assert list(status) == [J.OK, J.UNSUPPORTED, J.OK, J.CORRUPT, J.OK, J.RANGE]
    for n, out, s in zip(names, outs, status):
        if s == J.OK:
            assert np.array_equal(out, cases.pixels()[n]), n
        else:
            assert (out == 0xA5).all(), n


@pytest.mark.parametrize("size, names, given", [
    ((40, 56), ["40x56_420_q20.jpg", "40x56_444_q90.jpg", "40x56_grey_q90.jpg"], 1),
    # a 17 x 33 frame is 1683 bytes = 3 mod 4: frames 0 .. 3 begin 0, 3, 2 and 1 bytes past a dword
    # boundary and are all decoded, so every head of jpeg_colour's unaligned path is written
    ((17, 33), ["17x33_422_q90.jpg", "17x33_420_q20.jpg", "17x33_420_q90.jpg", "17x33_444_q20.jpg", "17x33_grey_q90.jpg"], 4),
])
def test_staged_frames_and_results_equal_staging_pillows_pixels(ctx, size, names, given):
    """op_jpeg_stage with one frame given as pixels: the staged set read back (draw_staged with empty
    display lists) is Pillow's pixels, and run_staged on it gives bit for bit the maps and results
    of run_staged after stage_frames(Pillow's pixels)."""
    render = pkg_module("render")
    h, w = size
    n = len(names)
    want = [cases.pixels()[k] for k in names]
    status = ctx.stage_jpegs([cases.files()[k] for k in names], h, w, [want[i] if i == given else None for i in range(n)])
    assert list(status) == [0] * n and ctx.staged_info() == (n, h, w)
    assert np.array_equal(render.render_staged(ctx, 0, n, [[]] * n), np.stack(want))
    ctx.run_staged()
    ctx.synchronize()
    maps, results = ctx.fetch_maps(0, n), ctx.fetch_results(0, n)
    ctx.stage_frames(np.stack(want))
    ctx.run_staged()
    ctx.synchronize()
    maps_ref, results_ref = ctx.fetch_maps(0, n), ctx.fetch_results(0, n)
    assert np.array_equal(maps[0], maps_ref[0]) and np.array_equal(maps[1], maps_ref[1])
    for (p, s, r), (p_ref, s_ref, r_ref) in zip(results, results_ref):
        assert np.array_equal(p, p_ref) and np.array_equal(s, s_ref)
        assert (r.status, r.n_peaks, r.n_persons) == (r_ref.status, r_ref.n_peaks, r_ref.n_persons)


def test_stage_statuses_and_zero_filled_slots(ctx):
    """A file of another size (OP_JPEG_SIZE), the progressive file and the truncated one staged with a
    good frame: their slots are zeros, the good frame is decoded as if they were absent."""
    J, render = pkg_module("jpeg"), pkg_module("render")
    names = ["bad_truncated.jpg", "40x56_422_q20.jpg", "37x45_420_q20.jpg", "bad_progressive.jpg"]
    status = ctx.stage_jpegs([cases.files()[n] for n in names], 40, 56)
    assert list(status) == [J.CORRUPT, J.OK, J.SIZE, J.UNSUPPORTED]
    got = render.render_staged(ctx, 0, 4, [[]] * 4)
    assert np.array_equal(got[1], cases.pixels()[names[1]])
    assert not got[0].any() and not got[2].any() and not got[3].any()


def test_stage_refusals(ctx, lib):
    """op_jpeg_stage's arguments are validated before any device call, and the staged set stays."""
    L, P = lib.lib(), lib.ptr
    good = np.frombuffer(cases.files()["40x56_422_q20.jpg"], np.uint8)
    ctx.stage_jpegs([cases.files()["40x56_422_q20.jpg"]], 40, 56)
    datas = (ctypes.c_void_p * 2)(good.ctypes.data, good.ctypes.data)
    sizes = (ctypes.c_int64 * 2)(len(good), len(good))
    null_second = (ctypes.c_void_p * 2)(good.ctypes.data, None)
    neg = (ctypes.c_int64 * 2)(len(good), -1)
    pix = np.zeros((40, 56, 3), np.uint8)
    first_given = (ctypes.c_void_p * 2)(pix.ctypes.data, None)
    status = np.full(2, -7, np.int32)
    for call, msg in (
            (lambda: L.op_jpeg_stage(ctx.h, 0, datas, sizes, None, 40, 56, P(status)), "n must be in 1 .. 65535"),
            (lambda: L.op_jpeg_stage(ctx.h, 65536, datas, sizes, None, 40, 56, P(status)), "n must be in 1 .. 65535"),
            (lambda: L.op_jpeg_stage(ctx.h, 2, datas, sizes, None, 4, 56, P(status)), "h, w must be in 8 .. 16384"),
            (lambda: L.op_jpeg_stage(ctx.h, 2, datas, sizes, None, 40, 16385, P(status)), "h, w must be in 8 .. 16384"),
            (lambda: L.op_jpeg_stage(ctx.h, 2, datas, sizes, None, 40, 56, None), "null status"),
            (lambda: L.op_jpeg_stage(ctx.h, 2, None, sizes, None, 40, 56, P(status)), "null data or bytes without bgr"),
            (lambda: L.op_jpeg_stage(ctx.h, 2, datas, None, None, 40, 56, P(status)), "null data or bytes without bgr"),
            (lambda: L.op_jpeg_stage(ctx.h, 2, None, None, first_given, 40, 56, P(status)), "frame 1: neither pixels nor a file"),
            (lambda: L.op_jpeg_stage(ctx.h, 2, null_second, sizes, first_given, 40, 56, P(status)), "data: frame 1: null file"),
            (lambda: L.op_jpeg_stage(ctx.h, 2, null_second, sizes, None, 40, 56, P(status)), "data: frame 1: null file"),
            (lambda: L.op_jpeg_stage(ctx.h, 2, datas, neg, None, 40, 56, P(status)), "bytes: frame 1: negative")):
        assert call() == lib.OP_ERR_INVALID and lib.last_error() == "op_jpeg_stage: " + msg, (msg, lib.last_error())
    assert (status == -7).all() and ctx.staged_info() == (1, 40, 56)
    with pytest.raises(ValueError):
        ctx.stage_jpegs([cases.files()["40x56_422_q20.jpg"]], 4, 56)


def test_run_staged_jpegs_routes_the_progressive_file_through_pillow(rand_weights):
    """A chunk with the progressive file (turned down by the probe) and a file past the range bound
    (turned down in the scan): 'host' for both, 'device' for the rest, the staged pixels and the
    results those of run_staged on Pillow's pixels."""
    J = pkg_module("jpeg")
    det = pkg_module("pose_detector").PoseDetector("posenet", model=rand_weights, max_batch=4)
    names = ["37x45_444_q20.jpg", "bad_progressive.jpg", "37x45_420_q75_restart_blocks2.jpg"]
    # the last file passes the probe and is turned down in the scan (OP_JPEG_RANGE): the second staging
    datas = [cases.files()[n] for n in names] + [cases.range_file()]
    n, routes = det.run_staged_jpegs(datas)
    assert n == 4 and routes == ["device", "host", "device", "host"]
    c = det.staged_context()
    c.synchronize()
    maps, results = c.fetch_maps(0, 4), c.fetch_results(0, 4)
    frames = np.stack([J.read_bgr_bytes(d) for d in datas])
    assert np.array_equal(frames[0], cases.pixels()[names[0]]) and frames.shape == (4, 37, 45, 3)
    assert np.array_equal(pkg_module("render").render_staged(c, 0, 4, [[]] * 4), frames)
    assert det.run_staged(frames) == 4
    c.synchronize()
    maps_ref, results_ref = c.fetch_maps(0, 4), c.fetch_results(0, 4)
    assert np.array_equal(maps[0], maps_ref[0]) and np.array_equal(maps[1], maps_ref[1])
    for (p, s, r), (p_ref, s_ref, r_ref) in zip(results, results_ref):
        assert np.array_equal(p, p_ref) and np.array_equal(s, s_ref) and r.n_persons == r_ref.n_persons
    with pytest.raises(ValueError):
        det.run_staged_jpegs(datas, size=(40, 56))


def test_eval_coco_device_jpeg_prints_the_same_summary(tmp_path, capsys):
    """eval_coco --random-weights on three JPEG images of two sizes (as tests/test_gpu_eval_coco_cli.py
    makes its dataset): the ten summary lines with --device-jpeg are those without it, and stderr says
    which route the frames took."""
    from PIL import Image
    cli = pkg_module("eval_coco")
    rng = np.random.default_rng(41)
    sizes = {1: (96, 128), 2: (128, 96), 5: (96, 128)}
    images, anns = [], []
    for img_id, (h, w) in sizes.items():
        name = "%012d.jpg" % img_id
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(str(tmp_path / name), quality=90)
        images.append({"id": img_id, "height": h, "width": w, "file_name": name})
    for img_id, size, visible in ((1, 60.0, 17), (1, 50.0, 9), (5, 70.0, 12)):
        kp = keypoint_cases.person(rng, 64, 48, size, visible).round()
        anns.append({"id": len(anns) + 1, "image_id": img_id, "category_id": 1, "iscrowd": 0,
                     "keypoints": [int(v) for v in kp.ravel()], "num_keypoints": visible, "area": size * size / 2,
                     "bbox": [64 - size / 2, 48 - size / 2, size, size]})
    path = tmp_path / "person_keypoints_tiny.json"
    path.write_text(json.dumps({"images": images, "annotations": anns, "categories": [{"id": 1, "name": "person"}]}))
    argv = ["--annotations", str(path), "--images", str(tmp_path), "--random-weights", "--batch", "2"]
    outs = []
    for flag in ([], ["--device-jpeg"]):
        results = tmp_path / ("results%d.json" % len(flag))
        assert cli.main(argv + flag + ["--results", str(results)]) == 0
        cap = capsys.readouterr()
        lines = [l for l in cap.out.splitlines() if l.startswith(" Average ")]
        assert len(lines) == 10
        outs.append((lines, json.loads(results.read_text())))
        said = [l for l in cap.err.splitlines() if l.startswith("device-jpeg:")]
        assert said == (["device-jpeg: 3 frames decoded on the device, 0 by Pillow on the host"] if flag else [])
    assert outs[0] == outs[1]
