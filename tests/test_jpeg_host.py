"""The JPEG decode without a GPU: jpeg.decode_np (the NumPy statement) against Pillow itself, the
host's C++ entropy decoder (op_jpeg_coefficients, op_jpeg_probe) against jpeg.coefficients_np /
jpeg.probe, the exactness predicate of the 32-bit inverse DCT, and the calls' argument validation."""
import ctypes
import io

import numpy as np
import pytest

import jpeg_cases as cases
from conftest import people_image, pkg_module


@pytest.fixture(scope="module")
def J():
    return pkg_module("jpeg")


def _pillow(data):
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[:, :, ::-1])


def _encode(bgr, sampling, **kw):
    from PIL import Image
    buf = io.BytesIO()
    img = Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1]))
    if sampling is None:
        img.convert("L").save(buf, "JPEG", **kw)
    else:
        img.save(buf, "JPEG", subsampling=sampling, **kw)
    return buf.getvalue()


def test_fixture_grid_is_complete():
    names = cases.positive()
    assert len(names) == 8 * 4 * 2 + 3 and set(cases.pixels()) == set(names)
    assert set(cases.NEGATIVE) <= set(cases.files())


@pytest.mark.parametrize("name", cases.positive())
def test_statement_equals_pillow_on_the_fixtures(J, name):
    data = cases.files()[name]
    want = cases.pixels()[name]
    assert np.array_equal(_pillow(data), want), "the stored pixels are not this Pillow's decode"
    got = cases.stated(name)
    assert got.shape == want.shape and got.dtype == np.uint8 and np.array_equal(got, want)


@pytest.mark.parametrize("sampling", [None, 0, 1, 2])
def test_statement_equals_pillow_on_fresh_encodes(J, sampling):
    """Sizes the fixtures do not hold (2 x 2, the 9 x 3 .. 9 x 6 run across the narrow-plane threshold,
    3 x 9, 33 x 50, 61 x 75), a photo crop and noise, qualities 10 .. 85."""
    photo = people_image()
    rng = np.random.default_rng(5)
    for k, (h, w) in enumerate([(2, 2), (9, 3), (9, 4), (9, 5), (9, 6), (3, 9), (33, 50), (35, 41), (61, 75)]):
        for q, img in ((10 + 25 * (k % 4), photo[50 + k:50 + k + h, 90:90 + w]), (85 - 25 * (k % 4), rng.integers(0, 256, (h, w, 3), dtype=np.uint8))):
            data = _encode(img, sampling, quality=q)
            assert np.array_equal(J.decode_np(data), _pillow(data)), (h, w, q)


@pytest.mark.parametrize("name", sorted(cases.files()))
def test_host_decoder_equals_the_stated_coefficients(J, lib, name):
    data = cases.files()[name]
    want = J.coefficients_np(data)
    status, info, coef, qt = lib.jpeg_coefficients(data)
    assert status == want["status"] == cases.NEGATIVE.get(name, 0)
    p = J.probe(data)
    assert p[0] == info.status and (info.status == 0 or (info.h, info.w, info.components, info.n_blocks) == (0, 0, 0, 0))
    if status != 0:
        return
    assert (info.h, info.w, info.components, (info.hs, info.vs)) == p[1:] == (want["h"], want["w"], want["components"], want["sampling"])
    nc = info.components
    assert [(info.blocks_h[c], info.blocks_w[c]) for c in range(nc)] == want["blocks"]
    assert [(info.blocks_h[c], info.blocks_w[c]) for c in range(nc, 3)] == [(0, 0)] * (3 - nc)
    assert info.n_blocks == sum(a * b for a, b in want["blocks"]) == len(coef)
    assert np.array_equal(qt[:nc], want["qt"]) and want["qt"].dtype == np.uint16
    assert coef.dtype == np.int16 and np.array_equal(coef, np.concatenate(want["coef"]))


def test_probe_statuses_of_the_negative_fixtures(J, lib):
    """Headers only: the progressive file is outside the subset, the random bytes are no JPEG; the
    truncated file's headers are whole (its scan is what fails: the decode says CORRUPT)."""
    want = {"bad_progressive.jpg": J.UNSUPPORTED, "bad_random.jpg": J.CORRUPT, "bad_truncated.jpg": J.OK}
    for name, status in want.items():
        data = cases.files()[name]
        assert J.probe(data)[0] == lib.jpeg_probe(data).status == status, name
    info = lib.jpeg_probe(cases.files()["bad_truncated.jpg"])
    assert (info.h, info.w, info.components, info.hs, info.vs) == (40, 56, 3, 2, 2)
    assert J.coefficients_np(cases.files()["bad_truncated.jpg"])["status"] == J.CORRUPT
    for data in (b"", b"\xff", b"\xff\xd8", b"\xff\xd8\xff\xd9", b"\x00" * 64):
        assert J.probe(data)[0] == lib.jpeg_probe(data).status == J.CORRUPT


def test_headers_outside_the_subset(J, lib):
    """Edits of a good file's headers: 12-bit precision, other sampling factors, other SOF kinds, a
    16-bit table, an Adobe segment are UNSUPPORTED; a missing table and a second SOF are CORRUPT."""
    good = cases.files()["16x16_420_q20.jpg"]
    sof = good.index(b"\xff\xc0")
    dqt = good.index(b"\xff\xdb")
    dht = good.index(b"\xff\xc4")
    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x01"

    def edit(at, value):
        return good[:at] + bytes([value]) + good[at + 1:]
    dht_len = (good[dht + 2] << 8) | good[dht + 3]
    sof_len = (good[sof + 2] << 8) | good[sof + 3]
    for data, status in ((edit(sof + 4, 12), J.UNSUPPORTED), (edit(sof + 11, 0x41), J.UNSUPPORTED),
                         (edit(sof + 11, 0x12), J.UNSUPPORTED), (edit(sof + 14, 0x21), J.UNSUPPORTED),
                         (edit(sof + 1, 0xc2), J.UNSUPPORTED), (edit(sof + 1, 0xc9), J.UNSUPPORTED),
                         (edit(dqt + 4, 0x10), J.UNSUPPORTED), (good[:2] + adobe + good[2:], J.UNSUPPORTED),
                         (good[:dht] + good[dht + 2 + dht_len:], J.CORRUPT),
                         (good[:sof] + good[sof:sof + 2 + sof_len] + good[sof:], J.CORRUPT),
                         (good[:2] + b"\xff\xe1\x00\x08Exif\x00\x00" + b"\xff\xfe\x00\x04hi" + good[2:], J.OK)):
        assert J.probe(data)[0] == lib.jpeg_probe(data).status == status, (data[:24], status)
        assert J.coefficients_np(data)["status"] == lib.jpeg_coefficients(data)[0] == status


def test_range_predicate_agrees_either_side_of_the_bound(J, lib):
    """sum |coef q| <= 32768: the statement's predicate and the host's, on blocks at the
    bound, one past it, far past it (int16 extremes times 255) and signed mixes."""
    rng = np.random.default_rng(9)
    q1 = np.ones(64, np.uint16)
    blocks = []
    for total in (0, 1, 32767, 32768, 32769, 40000):
        c = np.zeros(64, np.int64)
        c[0], c[1] = min(total, 30000), -(total - min(total, 30000))  # coefficients are int16
        blocks.append((c, q1, total <= 32768))
        parts = rng.multinomial(total, np.ones(64) / 64) * rng.choice([-1, 1], 64)
        blocks.append((parts, q1, total <= 32768))
    c = np.zeros(64, np.int64)
    c[5], c[63] = -128, 1
    blocks.append((c, np.full(64, 255, np.uint16), 129 * 255 <= 32768))  # 32895: past
    c = np.zeros(64, np.int64)
    c[5] = -128
    blocks.append((c, np.full(64, 255, np.uint16), True))  # 32640
    blocks.append((np.full(64, -32768, np.int64), np.full(64, 255, np.uint16), False))
    blocks.append((np.full(64, 32767, np.int64), np.full(64, 65535, np.uint16), False))
    for coef, q, want in blocks:
        assert J.in_range(coef, q) == lib.jpeg_block_in_range(coef, q) == want, (coef, q)
    assert J.IN_RANGE_SUM == 32768


def test_a_file_past_the_range_bound(J, lib):
    """A noise fixture with its quantisation tables set to 255: a well-formed file whose blocks sum far
    past the bound.  Both entropy decoders say RANGE with the same coefficients.  (Pillow decodes such
    a file to pixels of its own: libjpeg-turbo's vector inverse DCT saturates 16-bit lanes and its
    range limit masks where the statement clamps, so past the bound the 64-bit statement is not
    Pillow's output either -- the reason such frames take Pillow's route and are never guessed at.)"""
    data = cases.range_file()
    want = J.coefficients_np(data)
    status, info, coef, qt = lib.jpeg_coefficients(data)
    assert status == want["status"] == J.RANGE and J.probe(data)[0] == info.status == J.OK
    assert (qt == 255).all() and np.array_equal(coef, np.concatenate(want["coef"]))
    assert not all(J.in_range(b, qt[0]) for b in want["coef"][0])
    assert _pillow(data).shape == (37, 45, 3)  # still a file Pillow opens: the fallback has something to return


def test_statement_idct_fits_int32_at_the_bound(J):
    """The derivation's claim, checked on the statement: with sum |coef q| = 32768 put where it
    drives a pass hardest (one coefficient, every position and sign), every value either pass
    shifts down lies within int32, so 32-bit wrapping arithmetic gives the same samples."""
    worst = 0
    for k in range(64):
        for sign in (1, -1):
            x = np.zeros((1, 8, 8), np.int64)
            x.reshape(-1)[k] = sign * 32768
            raw1 = np.stack(J._idct_1d([x[:, i, :] for i in range(8)], 1), axis=1)  # shift 1: the sums, halved
            ws = np.stack(J._idct_1d([x[:, i, :] for i in range(8)], 11), axis=1)
            raw2 = np.stack(J._idct_1d([ws[:, :, i] for i in range(8)], 1), axis=2)
            worst = max(worst, 2 * int(np.abs(raw1).max()) + 1024, 2 * int(np.abs(raw2).max()) + (1 << 17))
    assert worst < 2 ** 31, worst
    assert 11363 * (11363 * 32768 // 2048 + 8) + (1 << 17) < 2 ** 31  # the bound DESIGN §23 derives


def test_argument_validation(lib):
    L = lib.lib()
    good = cases.files()["8x8_grey_q20.jpg"]
    buf = np.frombuffer(good, np.uint8)
    info = lib.OpJpegInfo()
    coef = np.zeros((4, 64), np.int16)
    qt = np.zeros((3, 64), np.uint16)
    st = ctypes.c_int32(-7)
    P = lib.ptr
    for rc, msg in (
            (lambda: L.op_jpeg_probe(None, 4, ctypes.byref(info)), "op_jpeg_probe: null data"),
            (lambda: L.op_jpeg_probe(P(buf), -1, ctypes.byref(info)), "op_jpeg_probe: negative bytes"),
            (lambda: L.op_jpeg_probe(P(buf), len(good), None), "op_jpeg_probe: null out"),
            (lambda: L.op_jpeg_coefficients(None, 4, P(coef), coef.size, P(qt), ctypes.byref(st)), "op_jpeg_coefficients: null data"),
            (lambda: L.op_jpeg_coefficients(P(buf), len(good), None, coef.size, P(qt), ctypes.byref(st)), "op_jpeg_coefficients: null coef"),
            (lambda: L.op_jpeg_coefficients(P(buf), len(good), P(coef), coef.size, None, ctypes.byref(st)), "op_jpeg_coefficients: null qt"),
            (lambda: L.op_jpeg_coefficients(P(buf), len(good), P(coef), coef.size, P(qt), None), "op_jpeg_coefficients: null status"),
            (lambda: L.op_jpeg_coefficients(P(buf), len(good), P(coef), 63, P(qt), ctypes.byref(st)),
             "op_jpeg_coefficients: coef_cap: 64 coefficients are needed"),
            (lambda: L.op_jpeg_block_in_range(None, P(qt), ctypes.byref(st)), "op_jpeg_block_in_range: null argument"),
            (lambda: L.op_jpeg_set_threads(65), "op_jpeg_set_threads: threads must be in 1 .. 64, or 0 for the default"),
            (lambda: L.op_jpeg_set_threads(-1), "op_jpeg_set_threads: threads must be in 1 .. 64, or 0 for the default"),
            (lambda: L.op_jpeg_set_threads(-3), "op_jpeg_set_threads: threads must be in 1 .. 64, or 0 for the default")):
        assert rc() == lib.OP_ERR_INVALID and lib.last_error() == msg, (msg, lib.last_error())
    assert L.op_jpeg_set_threads(1) == 0 and L.op_jpeg_set_threads(64) == 0 and L.op_jpeg_set_threads(0) == 0  # 0: the default again
    # op_jpeg_decode: everything is refused before a device is touched (there is none here)
    datas = (ctypes.c_void_p * 2)(buf.ctypes.data, buf.ctypes.data)
    sizes = (ctypes.c_int64 * 2)(len(good), len(good))
    out = np.zeros((2, 8, 8, 3), np.uint8)
    outs = (ctypes.c_void_p * 2)(out[0].ctypes.data, out[1].ctypes.data)
    status = np.full(2, -7, np.int32)
    null_second = (ctypes.c_void_p * 2)(buf.ctypes.data, None)
    out_null = (ctypes.c_void_p * 2)(out[0].ctypes.data, None)
    neg = (ctypes.c_int64 * 2)(len(good), -1)
    for rc, msg in (
            (lambda: L.op_jpeg_decode(0, -1, datas, sizes, outs, P(status)), "op_jpeg_decode: n must be in 0 .. 65535"),
            (lambda: L.op_jpeg_decode(0, 65536, datas, sizes, outs, P(status)), "op_jpeg_decode: n must be in 0 .. 65535"),
            (lambda: L.op_jpeg_decode(0, 2, None, sizes, outs, P(status)), "op_jpeg_decode: null data"),
            (lambda: L.op_jpeg_decode(0, 2, datas, None, outs, P(status)), "op_jpeg_decode: null bytes"),
            (lambda: L.op_jpeg_decode(0, 2, datas, sizes, None, P(status)), "op_jpeg_decode: null out"),
            (lambda: L.op_jpeg_decode(0, 2, datas, sizes, outs, None), "op_jpeg_decode: null status"),
            (lambda: L.op_jpeg_decode(0, 2, null_second, sizes, outs, P(status)), "op_jpeg_decode: data: frame 1: null file"),
            (lambda: L.op_jpeg_decode(0, 2, datas, neg, outs, P(status)), "op_jpeg_decode: bytes: frame 1: negative"),
            (lambda: L.op_jpeg_decode(0, 2, datas, sizes, out_null, P(status)), "op_jpeg_decode: out: frame 1: null image")):
        assert rc() == lib.OP_ERR_INVALID and lib.last_error() == msg, (msg, lib.last_error())
    assert not out.any() and (status == -7).all()
    assert L.op_jpeg_decode(0, 0, None, None, None, None) == 0  # nothing to do is not an error
    # no decodable frame: statuses, no device call, nothing written
    bad = np.frombuffer(cases.files()["bad_progressive.jpg"], np.uint8)
    datas = (ctypes.c_void_p * 2)(bad.ctypes.data, bad.ctypes.data)
    sizes = (ctypes.c_int64 * 2)(len(bad), 10)
    assert L.op_jpeg_decode(0, 2, datas, sizes, out_null, P(status)) == 0 and list(status) == [1, 2]
    # ... and nothing completed on a device: op_jpeg_last_ms has nothing to report for it
    assert L.op_jpeg_decode(62, 2, datas, sizes, out_null, P(status)) == 0
    assert L.op_jpeg_last_ms(62, (ctypes.c_double * 2)()) == lib.OP_ERR_STATE
    # op_jpeg_stage and op_jpeg_last_ms
    for rc, msg in (
            (lambda: L.op_jpeg_stage(None, 1, datas, sizes, None, 8, 8, P(status)), "op_jpeg_stage: null context"),
            (lambda: L.op_jpeg_last_ms(0, None), "op_jpeg_last_ms: null ms"),
            (lambda: L.op_jpeg_last_ms(-1, (ctypes.c_double * 2)()), "op_jpeg_last_ms: bad device -1"),
            (lambda: L.op_jpeg_last_ms(64, (ctypes.c_double * 2)()), "op_jpeg_last_ms: bad device 64")):
        assert rc() == lib.OP_ERR_INVALID and lib.last_error() == msg, (msg, lib.last_error())
    assert L.op_jpeg_last_ms(63, (ctypes.c_double * 2)()) == lib.OP_ERR_STATE
    assert lib.last_error() == "op_jpeg_last_ms: no op_jpeg_decode or op_jpeg_stage has completed on device 63"
