"""Baseline JPEG decode: the NumPy statement the device path is held to, and the calls into it.

The subset: baseline sequential DCT (SOF0), 8-bit samples, Huffman coding, one
interleaved scan, 8-bit quantisation tables, one component (grey) or three taken as YCbCr with luma
sampled 1x1, 2x1 or 2x2 and both chroma components 1x1; restart intervals and custom Huffman tables
are decoded, APPn / COM segments skipped.  Anything else gets a status and is left to Pillow:

    OK 0, UNSUPPORTED 1 (a well-formed file outside the subset), CORRUPT 2, SIZE 3 (staged call: not
    the h x w asked for), RANGE 4 (a block whose dequantised coefficients sum past IN_RANGE_SUM in
    magnitude: the kernel's 32-bit inverse DCT is exact only below it).

``decode_np`` states the whole decode in Python ints / int64 and equals
``np.asarray(Image.open(f).convert("RGB"))[:, :, ::-1]`` (libjpeg-turbo, JDCT_ISLOW, fancy
upsampling) byte for byte; ``coefficients_np`` states the entropy decode alone (what
csrc/jpeg_host.hpp computes on the host) and ``probe`` the header parse.  ``decode`` /
``decode_files`` run the HIP path (entropy decode on host threads, dequantisation, inverse DCT,
chroma upsampling and YCbCr -> BGR in csrc/jpeg.hip).
"""
import numpy as np

OK, UNSUPPORTED, CORRUPT, SIZE, RANGE = range(5)
MAX_SIDE = 16384
# sum over a block of |coef[k] * q[k]| up to which the 32-bit inverse DCT equals this statement
# (DESIGN §23 derives it)
IN_RANGE_SUM = 32768

ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
    28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
    54, 47, 55, 62, 63], np.int64)  # natural index of the k-th coefficient in zigzag order


def _fix(x):
    return int(round(x * 8192))


F_0_298631336, F_0_390180644, F_0_541196100, F_0_765366865 = _fix(0.298631336), _fix(0.390180644), _fix(0.541196100), _fix(0.765366865)
F_0_899976223, F_1_175875602, F_1_501321110, F_1_847759065 = _fix(0.899976223), _fix(1.175875602), _fix(1.501321110), _fix(1.847759065)
F_1_961570560, F_2_053119869, F_2_562915447, F_3_072711026 = _fix(1.961570560), _fix(2.053119869), _fix(2.562915447), _fix(3.072711026)
CONST_BITS, PASS1_BITS = 13, 2


class _Stop(Exception):
    def __init__(self, status):
        Exception.__init__(self, status)
        self.status = status


class _Header(object):
    """What the segments before the entropy-coded data say."""
    __slots__ = ("h", "w", "ncomp", "hs", "vs", "tq", "td", "ta", "qt", "huff", "ri", "ids", "scan", "bw", "bh")


def _huff_table(counts, symbols):
    """T.81 Annex C / F.2.2.3 -> (mincode[17], maxcode[17], valptr[17], symbols); CORRUPT when the
    code lengths overflow a prefix code."""
    mincode, maxcode, valptr = [0] * 17, [-1] * 17, [0] * 17
    code = k = 0
    for length in range(1, 17):
        valptr[length] = k
        mincode[length] = code
        code += counts[length - 1]
        k += counts[length - 1]
        if code > (1 << length):
            raise _Stop(CORRUPT)
        maxcode[length] = code - 1 if counts[length - 1] else -1
        code <<= 1
    return mincode, maxcode, valptr, symbols


def _parse(data):
    """The header parse (through the SOS header): -> _Header, or raises _Stop(status)."""
    data = bytes(data)
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise _Stop(CORRUPT)
    hd = _Header()
    hd.h = 0
    hd.ri = 0
    hd.qt = [None] * 4
    hd.huff = {}
    have_sof = False
    p = 2
    while True:
        if p >= n or data[p] != 0xFF:
            raise _Stop(CORRUPT)
        while p < n and data[p] == 0xFF:  # fill bytes
            p += 1
        if p >= n:
            raise _Stop(CORRUPT)
        m = data[p]
        p += 1
        if m in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xCB, 0xCC, 0xCD, 0xCE, 0xCF, 0xDC, 0xDE, 0xDF) \
                or 0xF0 <= m <= 0xFD:
            raise _Stop(UNSUPPORTED)
        if m in (0x00, 0x01, 0xD8, 0xD9) or 0xD0 <= m <= 0xD7 or m < 0xC0:
            raise _Stop(CORRUPT)
        if p + 2 > n:
            raise _Stop(CORRUPT)
        ln = (data[p] << 8) | data[p + 1]
        if ln < 2 or p + ln > n:
            raise _Stop(CORRUPT)
        seg = data[p + 2:p + ln]
        p += ln
        if m == 0xC0:
            if have_sof or len(seg) < 6:
                raise _Stop(CORRUPT)
            prec, h, w, nc = seg[0], (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if len(seg) != 6 + 3 * nc or w == 0 or nc == 0:
                raise _Stop(CORRUPT)
            if prec != 8 or h == 0 or nc not in (1, 3) or h > MAX_SIDE or w > MAX_SIDE:
                raise _Stop(UNSUPPORTED)
            ids = [seg[6 + 3 * i] for i in range(nc)]
            samp = [(seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15) for i in range(nc)]
            hd.tq = [seg[8 + 3 * i] for i in range(nc)]
            if any(not (1 <= a <= 4 and 1 <= b <= 4) for a, b in samp) or any(t > 3 for t in hd.tq):
                raise _Stop(CORRUPT)
            if len(set(ids)) != nc:
                raise _Stop(CORRUPT)
            if nc == 1:
                if samp[0] != (1, 1):
                    raise _Stop(UNSUPPORTED)
            elif samp[0] not in ((1, 1), (2, 1), (2, 2)) or samp[1] != (1, 1) or samp[2] != (1, 1) or ids == [82, 71, 66]:
                raise _Stop(UNSUPPORTED)
            hd.h, hd.w, hd.ncomp, (hd.hs, hd.vs) = h, w, nc, samp[0]
            hd.ids = ids
            have_sof = True
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                if q + 17 > len(seg):
                    raise _Stop(CORRUPT)
                tc, th = seg[q] >> 4, seg[q] & 15
                counts = list(seg[q + 1:q + 17])
                total = sum(counts)
                if tc > 1 or th > 3 or total > 256 or q + 17 + total > len(seg):
                    raise _Stop(CORRUPT)
                symbols = list(seg[q + 17:q + 17 + total])
                if tc == 0 and any(s > 15 for s in symbols):
                    raise _Stop(CORRUPT)
                hd.huff[(tc, th)] = _huff_table(counts, symbols)
                q += 17 + total
        elif m == 0xDB:
            q = 0
            while q < len(seg):
                pq, tq = seg[q] >> 4, seg[q] & 15
                if pq > 1 or tq > 3:
                    raise _Stop(CORRUPT)
                if pq == 1:
                    raise _Stop(UNSUPPORTED)
                if q + 65 > len(seg):
                    raise _Stop(CORRUPT)
                t = np.zeros(64, np.int64)
                t[ZIGZAG] = np.frombuffer(seg[q + 1:q + 65], np.uint8)
                hd.qt[tq] = t
                q += 65
        elif m == 0xDD:
            if len(seg) != 2:
                raise _Stop(CORRUPT)
            hd.ri = (seg[0] << 8) | seg[1]
        elif m == 0xEE:
            if len(seg) >= 12 and seg[:5] == b"Adobe":
                raise _Stop(UNSUPPORTED)
        elif m == 0xDA:
            if not have_sof or len(seg) < 1:
                raise _Stop(CORRUPT)
            ns = seg[0]
            if len(seg) != 4 + 2 * ns or ns < 1 or ns > 4:
                raise _Stop(CORRUPT)
            if ns != hd.ncomp or [seg[1 + 2 * i] for i in range(ns)] != hd.ids:
                raise _Stop(UNSUPPORTED)  # several scans, or components out of order
            hd.td = [seg[2 + 2 * i] >> 4 for i in range(ns)]
            hd.ta = [seg[2 + 2 * i] & 15 for i in range(ns)]
            if seg[1 + 2 * ns] != 0 or seg[2 + 2 * ns] != 63 or seg[3 + 2 * ns] != 0:
                raise _Stop(CORRUPT)
            for i in range(ns):
                if hd.td[i] > 3 or hd.ta[i] > 3 or (0, hd.td[i]) not in hd.huff or (1, hd.ta[i]) not in hd.huff \
                        or hd.qt[hd.tq[i]] is None:
                    raise _Stop(CORRUPT)  # a missing table
            mx, my = -(-hd.w // (8 * hd.hs)), -(-hd.h // (8 * hd.vs))
            hd.bw = [mx * hd.hs] + [mx] * (hd.ncomp - 1)
            hd.bh = [my * hd.vs] + [my] * (hd.ncomp - 1)
            blocks = sum(a * b for a, b in zip(hd.bw, hd.bh))
            if blocks > 4 * (n - p):  # a block takes two bits at the least
                raise _Stop(CORRUPT)
            hd.scan = p
            return hd
        # APPn, COM: skipped


def probe(data):
    """Headers only -> (status, h, w, components, (hs, vs) of the luma)."""
    try:
        hd = _parse(data)
    except _Stop as e:
        return e.status, 0, 0, 0, (0, 0)
    return OK, hd.h, hd.w, hd.ncomp, (hd.hs, hd.vs)


class _Bits(object):
    def __init__(self, data, p):
        self.d, self.p, self.acc, self.cnt = data, p, 0, 0

    def bit(self):
        if self.cnt == 0:
            d, p = self.d, self.p
            while True:
                if p >= len(d):
                    raise _Stop(CORRUPT)
                b = d[p]
                if b != 0xFF:
                    p += 1
                    break
                if p + 1 >= len(d):
                    raise _Stop(CORRUPT)
                if d[p + 1] == 0x00:
                    p += 2
                    break
                if d[p + 1] == 0xFF:  # a fill byte
                    p += 1
                    continue
                raise _Stop(CORRUPT)  # a marker where data was expected
            self.p, self.acc, self.cnt = p, b, 8
        self.cnt -= 1
        return (self.acc >> self.cnt) & 1

    def receive(self, s):
        v = 0
        for _ in range(s):
            v = (v << 1) | self.bit()
        return v

    def decode(self, table):
        mincode, maxcode, valptr, symbols = table
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            if maxcode[length] >= 0 and mincode[length] <= code <= maxcode[length]:
                return symbols[valptr[length] + code - mincode[length]]
        raise _Stop(CORRUPT)

    def marker(self):
        """The marker at the next byte boundary (fill bytes skipped), consumed; -1 without one."""
        self.cnt = 0
        d, p = self.d, self.p
        if p >= len(d) or d[p] != 0xFF:
            return -1
        while p < len(d) and d[p] == 0xFF:
            p += 1
        if p >= len(d) or d[p] == 0x00:
            return -1
        self.p = p + 1
        return d[p]


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def coefficients_np(data):
    """The entropy decode (T.81 F.2.2) -> dict: status, h, w, components, sampling (hs, vs) of the
    luma, blocks [(rows, columns) of each component's padded block grid], qt (components, 64) uint16
    in natural order, coef [per component (rows * columns, 64) int16: quantised coefficients in
    natural order, blocks in raster order].  With a status other than OK or RANGE only status is set."""
    data = bytes(data)
    try:
        hd = _parse(data)
        coef = [np.zeros((hd.bh[c] * hd.bw[c], 64), np.int16) for c in range(hd.ncomp)]
        br = _Bits(data, hd.scan)
        pred = [0] * hd.ncomp
        dc = [hd.huff[(0, t)] for t in hd.td]
        ac = [hd.huff[(1, t)] for t in hd.ta]
        qt = [hd.qt[t] for t in hd.tq]
        hs, vs = ([hd.hs, 1, 1], [hd.vs, 1, 1])
        mx, my = hd.bw[-1] if hd.ncomp > 1 else hd.bw[0], hd.bh[-1] if hd.ncomp > 1 else hd.bh[0]
        in_rng = True
        mcu, total, rst = 0, mx * my, 0
        for row in range(my):
            for col in range(mx):
                if hd.ri and mcu and mcu % hd.ri == 0:
                    if br.marker() != 0xD0 + (rst & 7):
                        raise _Stop(CORRUPT)
                    rst += 1
                    pred = [0] * hd.ncomp
                for c in range(hd.ncomp):
                    for v in range(vs[c]):
                        for u in range(hs[c]):
                            blk = coef[c][(row * vs[c] + v) * hd.bw[c] + col * hs[c] + u]
                            s = br.decode(dc[c])
                            pred[c] += _extend(br.receive(s), s)
                            if not -32768 <= pred[c] <= 32767:
                                raise _Stop(CORRUPT)
                            blk[0] = pred[c]
                            mag = abs(pred[c]) * int(qt[c][0])
                            k = 1
                            while k < 64:
                                rs = br.decode(ac[c])
                                r, s = rs >> 4, rs & 15
                                if s == 0:
                                    if r != 15:
                                        break
                                    k += 16
                                    if k > 64:
                                        raise _Stop(CORRUPT)
                                    continue
                                k += r
                                if k > 63:
                                    raise _Stop(CORRUPT)
                                val = _extend(br.receive(s), s)
                                blk[ZIGZAG[k]] = val
                                mag += abs(val) * int(qt[c][ZIGZAG[k]])
                                k += 1
                            in_rng = in_rng and mag <= IN_RANGE_SUM
                mcu += 1
        assert mcu == total
        if br.marker() != 0xD9:
            raise _Stop(CORRUPT)
    except _Stop as e:
        return {"status": e.status}
    return {"status": OK if in_rng else RANGE, "h": hd.h, "w": hd.w, "components": hd.ncomp, "sampling": (hd.hs, hd.vs),
            "blocks": list(zip(hd.bh, hd.bw)), "qt": np.stack(qt).astype(np.uint16), "coef": coef}


def in_range(coef, q):
    """The 32-bit inverse DCT's exactness predicate of one block: sum |coef[k] q[k]| <= IN_RANGE_SUM."""
    c = np.asarray(coef, np.int64).ravel()
    return int(np.abs(c * np.asarray(q, np.int64).ravel()).sum()) <= IN_RANGE_SUM


def _idct_1d(x, shift):
    """jidctint's 8-point pass on x[0..7] (int64 arrays), descaled by ``shift``."""
    z1 = (x[2] + x[6]) * F_0_541196100
    t2 = z1 - x[6] * F_1_847759065
    t3 = z1 + x[2] * F_0_765366865
    t0 = (x[0] + x[4]) << CONST_BITS
    t1 = (x[0] - x[4]) << CONST_BITS
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * F_1_175875602
    a0, a1, a2, a3 = a0 * F_0_298631336, a1 * F_2_053119869, a2 * F_3_072711026, a3 * F_1_501321110
    z1, z2 = z1 * -F_0_899976223, z2 * -F_2_562915447
    z3 = z3 * -F_1_961570560 + z5
    z4 = z4 * -F_0_390180644 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    out = (t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3)
    return [(v + (1 << (shift - 1))) >> shift for v in out]


def idct_np(coef, q):
    """(n, 64) quantised blocks and the (64,) table, natural order -> (n, 8, 8) uint8 samples."""
    x = (np.asarray(coef, np.int64) * np.asarray(q, np.int64)[None, :]).reshape(-1, 8, 8)
    ws = np.stack(_idct_1d([x[:, k, :] for k in range(8)], CONST_BITS - PASS1_BITS), axis=1)  # down the columns
    out = np.stack(_idct_1d([ws[:, :, k] for k in range(8)], CONST_BITS + PASS1_BITS + 3), axis=2)  # along the rows
    return np.clip(out + 128, 0, 255).astype(np.uint8)


def _upsample(s, hs, vs, h, w):
    """Chroma plane ``s`` (its true size) -> (h, w) int64, libjpeg's fancy filters (box at widths <= 2)."""
    s = s.astype(np.int64)
    ch, cw = s.shape
    if hs == 1 and vs == 1:
        return s[:h, :w]
    if cw <= 2:
        return np.repeat(np.repeat(s, vs, axis=0), hs, axis=1)[:h, :w]
    left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    if vs == 1:
        out = np.empty((ch, 2 * cw), np.int64)
        out[:, 0::2] = (3 * s + left + 1) >> 2
        out[:, 1::2] = (3 * s + right + 2) >> 2
        return out[:h, :w]
    up = np.concatenate([s[:1], s[:-1]], axis=0)
    down = np.concatenate([s[1:], s[-1:]], axis=0)
    out = np.empty((2 * ch, 2 * cw), np.int64)
    for k, other in ((0, up), (1, down)):
        v = 3 * s + other
        vl = np.concatenate([v[:, :1], v[:, :-1]], axis=1)
        vr = np.concatenate([v[:, 1:], v[:, -1:]], axis=1)
        out[k::2, 0::2] = (3 * v + vl + 8) >> 4
        out[k::2, 1::2] = (3 * v + vr + 7) >> 4
    return out[:h, :w]


def _f16(x):
    return int(x * 65536 + 0.5)


def pixels_np(c):
    """``coefficients_np``'s record (status OK) -> (h, w, 3) uint8 BGR."""
    h, w, hs, vs = c["h"], c["w"], c["sampling"][0], c["sampling"][1]
    planes = []
    for i in range(c["components"]):
        bh, bw = c["blocks"][i]
        p = idct_np(c["coef"][i], c["qt"][i]).reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)
        planes.append(p)
    y = planes[0][:h, :w].astype(np.int64)
    if c["components"] == 1:
        return np.repeat(y.astype(np.uint8)[:, :, None], 3, axis=2)
    ch, cw = -(-h // vs), -(-w // hs)
    cb = _upsample(planes[1][:ch, :cw], hs, vs, h, w) - 128
    cr = _upsample(planes[2][:ch, :cw], hs, vs, h, w) - 128
    r = y + ((_f16(1.40200) * cr + 32768) >> 16)
    b = y + ((_f16(1.77200) * cb + 32768) >> 16)
    g = y + ((-_f16(0.34414) * cb - _f16(0.71414) * cr + 32768) >> 16)
    return np.clip(np.stack([b, g, r], axis=2), 0, 255).astype(np.uint8)


def decode_np(data):
    """The decode, stated: file bytes -> (h, w, 3) uint8 BGR (ValueError outside the subset)."""
    c = coefficients_np(data)
    if c["status"] != OK:  # RANGE too: past the bound libjpeg-turbo's own arithmetic leaves this statement
        raise ValueError("jpeg.decode_np: status %d" % c["status"])
    return pixels_np(c)


def read_bgr_bytes(data):
    """``draw.read_bgr``'s method on file bytes (Pillow): the route of every frame outside the subset."""
    import io
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(bytes(data))).convert("RGB"))[:, :, ::-1])


def file_bytes(item):
    """bytes-like stays, a path is read."""
    if isinstance(item, (bytes, bytearray, memoryview)):
        return bytes(item)
    with open(item, "rb") as f:
        return f.read()


def decode(datas, device=0):
    """Decode a batch of files on the device in one call (op_jpeg_decode; any mix of sizes and
    samplings) -> (list of (h, w, 3) uint8 BGR arrays, None where the status is not OK; statuses)."""
    from . import _lib
    datas = [bytes(d) for d in datas]
    infos = [_lib.jpeg_probe(d) for d in datas]
    outs = [np.empty((i.h, i.w, 3), np.uint8) if i.status == OK else None for i in infos]
    status = _lib.jpeg_decode(datas, outs, device)
    return [o if s == OK else None for o, s in zip(outs, status)], [int(s) for s in status]


def decode_files(paths, device=0):
    """Files -> list of BGR arrays: the device path, Pillow for every frame it turns down.
    -> (frames, routes) with routes[i] 'device' or 'host'."""
    datas = [file_bytes(p) for p in paths]
    frames, status = decode(datas, device)
    routes = []
    for i, s in enumerate(status):
        routes.append("device" if s == OK else "host")
        if s != OK:
            frames[i] = read_bgr_bytes(datas[i])
    return frames, routes
