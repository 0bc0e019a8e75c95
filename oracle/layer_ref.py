"""ORACLE — TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

Single-layer reference for the probe points of ``op_forward_probe`` (include/openpose_hip.h): the
layer, or fused group of layers, between two probe points, evaluated in float64 at chosen output
pixels from the input the GPU actually gave it.  Our own NumPy code; nothing here is a restatement
of the reference project beyond the layer wiring of models/CocoPoseNet.py:132-262 and, for
``net="facenet"`` / ``"handnet"`` (the points of ``op_cpm_forward_probe``), of models/FaceNet.py:78-161
/ models/HandNet.py:78-161, written down here as a table of our own (``_cpm_point_spec``) over the
layer names of ``op_cpm_layer_info``.  The CPM nets run in bf16x3 only, conv1_1 in its ``"mfma"`` form
(csrc/cpm.hip cpm_run calls launch_conv1_pair).

Two precisions, as ``op_set_precision``:

* ``fp32``: the ideal is ``sum(w x) + b`` (then ReLU / 2x2 max-pool).
* ``bf16x3``: every operand is the pair ``(hi, lo) = (bf16(v), bf16(v - hi))`` (``split`` below =
  csrc/host_pack.hpp ``bf16_rne`` / ``pack_split`` for the weights, the kernels' epilogues for the
  activations, e.g. conv_bf16x3.hip ``store_tile``) and a product is the three terms the kernels form,
  ``w_hi x_hi + w_hi x_lo + w_lo x_hi`` (conv_bf16x3.hip: the three MFMAs per (chunk, tap) step).
  The dropped ``w_lo x_lo`` is of the order of the tolerance and therefore is NOT part of the ideal.

Fused groups compose their steps and round the intermediate the way the kernels do:

* point 1 (conv1_1 + conv1_2 + pool): conv1_1's output goes through ReLU and the hi/lo split before
  conv1_2 reads it (conv1_pair.hip, the ``hv`` / ``lv`` stores into the LDS planes; conv11.hip's epilogue
  for the two-kernel path).  ``conv11="mfma"`` (conv1_pair.hip, C1P_MFMA11): conv1_1 is itself three
  bf16 products per MAC on weights split in the kernel, and its bias rides in the accumulation
  (K slot 27, B = 1.0) as the split pair ``bf16(b) + bf16(b - hi)``; ``conv11="f32"`` (conv11.hip, the path
  of the other conv algos): f32 FMAs on the unsplit weights, ``sum(w x) + b``.
* pooled points: max over the 2x2 window of the ReLU'd conv (conv1_pair.hip / conv_m16k.hpp pool
  epilogues; maxpool2_split compares reconstructed values, so the order of pool and split does not
  matter beyond the output rounding the tolerance carries).
* the heads (conv5_4 + conv5_5, Mconv6 + Mconv7): the first 1x1's output goes through bias, ReLU and
  the hi/lo split (conv_head.hip, "bias + ReLU + split -> T[px][chunk channel]"); in fp32 it stays
  f32 (conv.hip conv_head_f32).

``seq_f32`` evaluates the same terms in float32, added one at a time in (16-channel chunk, tap,
product, channel) order, the chunks being those of the kernels' physical channel layout: the accumulation-error yardstick ``e_seq`` of the tolerance

    |y_gpu - ideal| <= 2 e_seq + r |ideal|,   r = 2^-17 (split-stored) or 2^-23 (f32).
"""
import numpy as np

R_SPLIT = 2.0 ** -17
R_F32 = 2.0 ** -23
N_POINTS = 46
MAP_POINTS = (15, 21, 27, 33, 39, 45)


def bf16_rne(x):
    """float32 -> the nearest bf16 (ties to even; inf / nan truncated), returned as float32:
    csrc/host_pack.hpp bf16_rne followed by bf16_f."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32)
    special = (u & np.uint32(0x7F800000)) == np.uint32(0x7F800000)
    r = u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))
    r = np.where(special, u, r) & np.uint32(0xFFFF0000)
    return r.astype(np.uint32).view(np.float32).reshape(x.shape)


def split(x):
    """(hi, lo) = (bf16(x), bf16(x - hi)) as float32 arrays (host_pack.hpp pack_split; store_tile)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hi = bf16_rne(x)
    lo = bf16_rne(x - hi)
    return hi, lo


def recon(x):
    """What a split store keeps of x: hi + lo (exact in float32)."""
    hi, lo = split(x)
    return hi + lo


NETS = ("posenet", "facenet", "handnet")
CPM_MAPS = {"facenet": 71, "handnet": 22}  # C: the heat maps of models/FaceNet.py / models/HandNet.py
CPM_FEATURE_POINT = 14  # conv5_3_CPM, the 128-channel feature map (posenet: point 11)


def cpm_heat_channels(net):
    """Channels of the heat slice a CPM map point returns: the stage buffer's 128 + C channels are
    padded to a multiple of 16 (csrc/cpm.hip cat_cs), 80 for facenet and 32 for handnet; those from C
    on are zero."""
    return (128 + CPM_MAPS[net] + 15) // 16 * 16 - 128


def _cpm_point_spec(point, net):
    """The launches of csrc/cpm.hip cpm_run between two probe points.  Mconv1 of stage s reads the
    logical concat (heat C, feature 128) out of the probed map point [heat C | zero pad | feature 128]:
    its channel selector is an index array instead of a (c0, c1) slice."""
    C = CPM_MAPS[net]
    one = {2: "conv2_1", 4: "conv3_1", 5: "conv3_2", 6: "conv3_3", 8: "conv4_1", 9: "conv4_2", 10: "conv4_3",
           11: "conv4_4", 12: "conv5_1", 13: "conv5_2", 14: "conv5_3_CPM"}
    pooled = {3: "conv2_2", 7: "conv3_4"}
    if point == 1:
        return 0, [([("conv1_1", 0, 3)], True), ([("conv1_2", 0, 64)], True)], True
    if point in one:
        return point - 1, [([(one[point], 0, None)], True)], False
    if point in pooled:
        return point - 1, [([(pooled[point], 0, None)], True)], True
    if point == 15:
        return 14, [([("conv6_1_CPM", 0, 128)], True), ([("conv6_2_CPM", 0, 512)], False)], False
    s, i = 2 + (point - 16) // 6, (point - 16) % 6
    if i == 0:
        sel = np.concatenate([np.arange(C), cpm_heat_channels(net) + np.arange(128)]).astype(np.int64)
        return point - 1, [([("Mconv1_stage%d" % s, sel, None)], True)], False
    if i < 5:
        return point - 1, [([("Mconv%d_stage%d" % (i + 1, s), 0, 128)], True)], False
    return point - 1, [([("Mconv6_stage%d" % s, 0, 128)], True), ([("Mconv7_stage%d" % s, 0, 128)], False)], False


def point_spec(point, net="posenet"):
    """-> (input point, steps, pooled).  steps: [(groups, relu)], groups: [(layer, c0, c1)] = the layer
    reads input channels [c0, c1) (c0 an index array: those channels) and the groups' outputs are
    concatenated.  The map points' steps give the 57 (paf | heat) channels (C heat channels for the
    CPM nets); the probe appends the 128 feature channels (a copy of point 11; 14 for the CPM nets,
    behind the heat slice's zero padding)."""
    if net not in NETS:
        raise ValueError("net: one of %s" % (NETS,))
    if not 1 <= point < N_POINTS:
        raise ValueError("point 1 .. 45")
    if net != "posenet":
        return _cpm_point_spec(point, net)
    one = {2: "conv2_1", 4: "conv3_1", 5: "conv3_2", 6: "conv3_3", 8: "conv4_1", 9: "conv4_2", 10: "conv4_3_CPM",
           11: "conv4_4_CPM"}
    pooled = {3: "conv2_2", 7: "conv3_4"}
    if point == 1:
        return 0, [([("conv1_1", 0, 3)], True), ([("conv1_2", 0, 64)], True)], True
    if point in one:
        return point - 1, [([(one[point], 0, None)], True)], False
    if point in pooled:
        return point - 1, [([(pooled[point], 0, None)], True)], True
    if point == 12:
        return 11, [([("conv5_1_CPM_L1", 0, 128), ("conv5_1_CPM_L2", 0, 128)], True)], False
    if point in (13, 14):
        i = point - 11
        return point - 1, [([("conv5_%d_CPM_L1" % i, 0, 128), ("conv5_%d_CPM_L2" % i, 128, 256)], True)], False
    if point == 15:
        return 14, [([("conv5_4_CPM_L1", 0, 128), ("conv5_4_CPM_L2", 128, 256)], True),
                    ([("conv5_5_CPM_L1", 0, 512), ("conv5_5_CPM_L2", 512, 1024)], False)], False
    s, i = 2 + (point - 16) // 6, (point - 16) % 6
    if i == 0:
        return point - 1, [([("Mconv1_stage%d_L1" % s, 0, 185), ("Mconv1_stage%d_L2" % s, 0, 185)], True)], False
    if i < 5:
        return point - 1, [([("Mconv%d_stage%d_L1" % (i + 1, s), 0, 128),
                             ("Mconv%d_stage%d_L2" % (i + 1, s), 128, 256)], True)], False
    return point - 1, [([("Mconv6_stage%d_L1" % s, 0, 128), ("Mconv6_stage%d_L2" % s, 128, 256)], True),
                       ([("Mconv7_stage%d_L1" % s, 0, 128), ("Mconv7_stage%d_L2" % s, 128, 256)], False)], False


def out_channels(point, weights, net="posenet"):
    """Channels the point's layers write (57, or C, at the map points, without the feature copy)."""
    groups = point_spec(point, net)[1][-1][0]
    return sum(weights[name][0].shape[0] for name, _, _ in groups)


class _Run(object):
    def __init__(self, precision, inputs, weights, mode, conv11, mutate, reverse=False, net="posenet", inputs_hi=None):
        self.net = net
        # the hi halves of the stored input pairs (bf16x3): the operands are then (hi, inputs - hi) and a
        # fused group's intermediate keeps the pair the kernel makes, instead of split(hi + lo)
        self.x_hi = None if inputs_hi is None else np.ascontiguousarray(inputs_hi, dtype=np.float32)
        if precision not in ("fp32", "bf16x3"):
            raise ValueError("precision: 'fp32' or 'bf16x3'")
        if conv11 not in ("mfma", "f32"):
            raise ValueError("conv11: 'mfma' or 'f32'")
        self.split = precision == "bf16x3"
        self.x = np.ascontiguousarray(inputs, dtype=np.float32)
        self.w = weights
        self.seq = mode == "seq"
        self.conv11 = conv11
        self.mutate = mutate or {}
        self.reverse = reverse


def _operands(xm, xm_hi):
    """The (hi, lo) pair of the activations: the stored one where its hi halves are known, else split()
    of hi + lo -- the same pair unless hi + lo lies exactly halfway between two bf16 values (0.1 % of
    the stored values): the kernel that stored it rounded its f32 value, which was off the tie, to
    either neighbour and lo to minus or plus half a step, and split() of the sum always takes the even
    one.  The three products differ between the two pairs by w_lo times one bf16 step of x."""
    if xm_hi is None:
        return split(xm)
    return xm_hi, xm - xm_hi  # exact: lo is a bf16 value


def _gemm_ideal(run, name, xg, W, b, last, xg_hi=None):
    """xg (P, taps, Ci) f32, W (taps, Ci, Co) f32 -> (P, Co) float64."""
    P = xg.shape[0]
    K = W.shape[0] * W.shape[1]
    Wm = W.reshape(K, -1)
    xm = xg.reshape(P, K)
    bias = b.astype(np.float64)
    exact = (not run.split) or (name == "conv1_1" and run.conv11 == "f32")
    if exact:
        return xm.astype(np.float64) @ Wm.astype(np.float64) + bias
    x_hi, x_lo = _operands(xm, None if xg_hi is None else xg_hi.reshape(P, K))
    w_hi, w_lo = split(Wm)
    x_hi, x_lo, w_hi, w_lo = (a.astype(np.float64) for a in (x_hi, x_lo, w_hi, w_lo))
    drop = run.mutate.get("drop") if last else None
    if drop is None:
        y = (x_hi + x_lo) @ w_hi + x_hi @ w_lo  # hi + lo is exact in float64
    else:
        y = x_hi @ w_hi
        if drop != "w_hi*x_lo":
            y += x_lo @ w_hi
        if drop != "w_lo*x_hi":
            y += x_hi @ w_lo
    if name == "conv1_1":  # conv1_pair.hip: K slot 27 carries the bias as A = split(b11), B = 1.0
        bias = recon(b).astype(np.float64)
    return y + bias


def _physical_channels(net, name, ci):
    """src[p] = the logical input channel of `name` at physical channel p of the tensor the kernels
    walk, -1 for channel padding; None where the two orders are the same.
    posenet (185 channels): feature at 0..127, heat at 128..146, paf at 152..189 of 192 (csrc/common.hpp
    kCatFeat / kCatHeat / kCatPaf; weights.hip cat_logical).  CPM Mconv1 (C + 128 channels): feature at
    0..127, heat at 128..128+C-1 of 128 + C rounded up to 16 (csrc/cpm.hip op_cpm_set_weights cmap):
    feature chunks 0..7, then the heat chunks; 9 of the 16 channels of facenet's 13th chunk are padding."""
    if net == "posenet":
        if ci != 185:
            return None
        src = np.full(192, -1, np.int64)
        src[0:128] = np.arange(57, 185)
        src[128:147] = np.arange(38, 57)
        src[152:190] = np.arange(0, 38)
        return src
    C = CPM_MAPS[net]
    if not name.startswith("Mconv1_") or ci != C + 128:
        return None
    src = np.full(128 + cpm_heat_channels(net), -1, np.int64)
    src[0:128] = C + np.arange(128)
    src[128:128 + C] = np.arange(C)
    return src


def _kernel_channel_order(run, name, xg, W):
    """The stage input in the order the kernels walk it (_physical_channels), zeros at the padding.
    posenet: the 185-channel stage input in the order the kernels walk it: a 192-channel pixel with the
    feature at 0..127, heat at 128..146 and paf at 152..189, zeros between (csrc/common.hpp kCatFeat /
    kCatHeat / kCatPaf; weights.hip cat_logical packs Mconv1's weights the same way).  The order is
    part of the yardstick: measured on the GPU in fp32, Mconv1's error has the r.m.s. of the
    sequential sum in this order, 25 % above that of the (paf, heat, feature) order."""
    src = _physical_channels(run.net, name, xg.shape[2])
    if src is None:
        return xg, W
    xp = np.zeros(xg.shape[:2] + (len(src),), xg.dtype)
    Wp = np.zeros((W.shape[0], len(src), W.shape[2]), W.dtype)
    xp[:, :, src >= 0] = xg[:, :, src[src >= 0]]
    Wp[:, src >= 0] = W[:, src[src >= 0]]
    return xp, Wp


def _gemm_seq(run, name, xg, W, b, xg_hi=None):
    """The same terms in float32, one at a time: 16-channel chunk, tap, product, channel.  A bf16 x
    bf16 product is exact in float32, so only the adds round; on the exact paths every term is one
    fused multiply-add (the float64 product of two float32 is exact)."""
    if xg_hi is not None:
        xg_hi = _kernel_channel_order(run, name, xg_hi, W)[0]
    xg, W = _kernel_channel_order(run, name, xg, W)
    if run.reverse:  # the channels walked backwards: the same sum in another order
        xg, W = xg[:, :, ::-1], W[:, ::-1]
        xg_hi = None if xg_hi is None else xg_hi[:, :, ::-1]
    P, taps, Ci = xg.shape
    Co = W.shape[2]
    acc = np.zeros((P, Co), np.float32)
    exact = (not run.split) or (name == "conv1_1" and run.conv11 == "f32")
    if exact:
        x64, w64 = xg.astype(np.float64), W.astype(np.float64)
        for c0 in range(0, Ci, 16):
            for t in range(taps):
                for ci in range(c0, min(c0 + 16, Ci)):
                    acc = (acc + x64[:, t, ci, None] * w64[t, ci][None, :]).astype(np.float32)
        return (acc + b.astype(np.float32)[None, :]).astype(np.float64)
    x_hi, x_lo = _operands(xg, xg_hi)
    w_hi, w_lo = split(W)
    for c0 in range(0, Ci, 16):
        c1 = min(c0 + 16, Ci)
        for t in range(taps):
            for xa, wa in ((x_hi, w_hi), (x_lo, w_hi), (x_hi, w_lo)):
                for ci in range(c0, c1):
                    acc = acc + xa[:, t, ci, None] * wa[t, ci][None, :]
    bias = recon(b) if name == "conv1_1" else b.astype(np.float32)
    return (acc + bias[None, :]).astype(np.float64)


def _eval(run, steps, k, pix):
    """Step k's output (after its ReLU) at pixels pix (P, 3: frame, y, x) -> (P, C) float64."""
    F, C, H, Wd = run.x.shape
    groups, relu = steps[k]
    last = k == len(steps) - 1
    ks = run.w[groups[0][0]][0].shape[2]
    R = ks // 2
    P = pix.shape[0]
    dy, dx = np.meshgrid(np.arange(ks) - R, np.arange(ks) - R, indexing="ij")
    shift = int(run.mutate.get("shift", 0)) if last else 0
    ny = pix[:, 1, None] + dy.reshape(1, -1)
    nx = pix[:, 2, None] + dx.reshape(1, -1) + shift
    inside = (ny >= 0) & (ny < H) & (nx >= 0) & (nx < Wd)
    code = (pix[:, 0, None] * H + np.where(inside, ny, 0)) * Wd + np.where(inside, nx, 0)
    uniq, inv = np.unique(code[inside], return_inverse=True)
    upix = np.stack([uniq // (H * Wd), (uniq // Wd) % H, uniq % Wd], axis=1)
    prev_hi = None
    if k == 0:
        prev = run.x[upix[:, 0], :, upix[:, 1], upix[:, 2]]  # (U, C) f32
        if run.x_hi is not None and run.split:
            prev_hi = run.x_hi[upix[:, 0], :, upix[:, 1], upix[:, 2]]
    else:
        prev = _eval(run, steps, k - 1, upix).astype(np.float32)  # the kernel's f32 value ...
        if run.split:
            if run.x_hi is not None:
                prev_hi = bf16_rne(prev)  # (the pair the kernel makes of it)
            prev = recon(prev)  # ... kept as its hi/lo pair
    prev = np.concatenate([prev, np.zeros((1, prev.shape[1]), np.float32)], axis=0)  # row U: zero padding
    if prev_hi is not None:
        prev_hi = np.concatenate([prev_hi, np.zeros((1, prev_hi.shape[1]), np.float32)], axis=0)
    idx = np.full(code.shape, len(uniq), np.int64)
    idx[inside] = inv
    out = []
    for name, c0, c1 in groups:
        Wl, b = run.w[name]
        Wt = np.ascontiguousarray(np.asarray(Wl, np.float32).transpose(2, 3, 1, 0)).reshape(ks * ks, Wl.shape[1], Wl.shape[0])
        pg = prev[:, c0] if isinstance(c0, np.ndarray) else prev[:, c0:c1]
        pg_hi = None if prev_hi is None else (prev_hi[:, c0] if isinstance(c0, np.ndarray) else prev_hi[:, c0:c1])
        ys = []
        blk = max(1, (32 << 20) // (ks * ks * pg.shape[1] * 4))
        for p0 in range(0, P, blk):
            xg = pg[idx[p0:p0 + blk]]  # (p, taps, Ci)
            xg_hi = None if pg_hi is None else pg_hi[idx[p0:p0 + blk]]
            if last and "chunk" in run.mutate:
                pi, tap, c16 = run.mutate["chunk"]
                if run.net != "posenet":  # the CPM nets: chunk c16 of the physical order
                    phys = _physical_channels(run.net, name, xg.shape[2])
                    lost = (phys if phys is not None else np.arange(xg.shape[2]))[16 * c16:16 * c16 + 16]
                    if p0 <= pi < p0 + blk:
                        xg = xg.copy()
                        xg[pi - p0, tap, lost[lost >= 0]] = 0
                        if xg_hi is not None:
                            xg_hi = xg_hi.copy()
                            xg_hi[pi - p0, tap, lost[lost >= 0]] = 0
                elif p0 <= pi < p0 + blk and c0 <= 16 * c16 < (c1 if c1 is not None else 1 << 30):
                    xg = xg.copy()
                    xg[pi - p0, tap, 16 * c16 - c0:16 * c16 - c0 + 16] = 0
            b = np.asarray(b, np.float32)
            ys.append(_gemm_seq(run, name, xg, Wt, b, xg_hi) if run.seq else _gemm_ideal(run, name, xg, Wt, b, last, xg_hi))
        out.append(np.concatenate(ys, axis=0))
    y = np.concatenate(out, axis=1)
    return np.maximum(y, 0.0) if relu else y


def _evaluate(point, precision, inputs, weights, pixels, mode, conv11, mutate, reverse=False, net="posenet",
              inputs_hi=None):
    run = _Run(precision, inputs, weights, mode, conv11, mutate, reverse, net, inputs_hi)
    _, steps, pooled = point_spec(point, net)
    pix = np.asarray(pixels, np.int64).reshape(-1, 3)
    if not pooled:
        return _eval(run, steps, len(steps) - 1, pix)
    quad = []
    for a in (0, 1):
        for b in (0, 1):
            quad.append(_eval(run, steps, len(steps) - 1, pix * np.array([1, 2, 2]) + np.array([0, a, b])))
    return np.maximum(np.maximum(quad[0], quad[1]), np.maximum(quad[2], quad[3]))


def ideal(point, precision, inputs, weights, pixels, conv11="mfma", mutate=None, net="posenet", inputs_hi=None):
    """The float64 ideal of probe point `point` at output pixels `pixels` ((P, 3): frame, y, x of the
    point's output map) from `inputs` (frames, C, H, W): the probed tensor of point_spec(point)[0] (its
    first C channels are read; a map point's 185 are what Mconv1 reads).  -> (P, channels) float64.
    mutate (the sensitivity tests): {"drop": "w_lo*x_hi" | "w_hi*x_lo"}, {"shift": 1} (the patch one
    column to the right), {"chunk": (pixel index, tap, 16-channel chunk)} (those products lost; for the
    CPM nets the chunk of the physical channel order, _physical_channels).
    net "facenet" / "handnet": the points of op_cpm_forward_probe; a map point's tensor is [heat C |
    zero pad | feature 128] as probed, of which Mconv1 reads the (heat C, feature 128) channels.
    inputs_hi (bf16x3): the hi halves of the stored input pairs, as the probe returns them on request
    (_operands says why hi + lo alone is not enough); with them a fused group's intermediate also
    keeps the kernel's own pair.  Without, every pair is split() of the value."""
    return _evaluate(point, precision, inputs, weights, pixels, "ideal", conv11, mutate, net=net, inputs_hi=inputs_hi)


def seq_f32(point, precision, inputs, weights, pixels, conv11="mfma", reverse=False, net="posenet", inputs_hi=None):
    """The same terms as ideal() accumulated in float32 one at a time (16-channel chunk, tap, product,
    channel order), fused groups composed the same way: the accumulation-error yardstick.  reverse:
    the channels walked backwards, i.e. another correct accumulation (tests/test_layer_ref.py holds
    the yardstick to it)."""
    return _evaluate(point, precision, inputs, weights, pixels, "seq", conv11, None, reverse, net, inputs_hi)


def all_pixels(frames, h, w):
    """(frames h w, 3) int64: every (frame, y, x) in raster order."""
    f, y, x = np.meshgrid(np.arange(frames), np.arange(h), np.arange(w), indexing="ij")
    return np.stack([f.ravel(), y.ravel(), x.ravel()], axis=1).astype(np.int64)


def to_nchw(values, frames, h, w):
    """(frames h w, C) values at all_pixels(frames, h, w) -> (frames, C, h, w)."""
    return np.ascontiguousarray(values.reshape(frames, h, w, -1).transpose(0, 3, 1, 2))


def walk(weights, x, precision, upto, conv11="mfma", net="posenet"):
    """{point: (frames, C, h, w) float32} for points 0 .. upto: every point's ideal at every pixel from
    the previous point's stored result (float32; its hi + lo in bf16x3), the map points with the
    feature copy appended (for the CPM nets behind the heat slice's zero padding, as probed) -- tensors
    with the statistics of the probed ones, for the CPU tests."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    acts = {0: recon(x) if precision == "bf16x3" else x}
    for p in range(1, upto + 1):
        src, _, pooled = point_spec(p, net)
        inp = acts[src]
        F, _, H, W = inp.shape
        oh, ow = (H // 2, W // 2) if pooled else (H, W)
        y = ideal(p, precision, inp, weights, all_pixels(F, oh, ow), conv11, net=net).astype(np.float32)
        y = to_nchw(recon(y) if precision == "bf16x3" else y, F, oh, ow)
        if p in MAP_POINTS and net != "posenet":
            pad = np.zeros((F, cpm_heat_channels(net) - y.shape[1], oh, ow), np.float32)
            y = np.concatenate([y, pad, acts[CPM_FEATURE_POINT]], axis=1)
        elif p in MAP_POINTS:
            y = np.concatenate([y, acts[11]], axis=1)
        acts[p] = y
    return acts


def yardstick_pixels(ideal_values, ksize, rng):
    """Indices (into the rows of ideal_values (P, C)) of the pixels seq_f32 is evaluated at.  The error
    of a running f32 sum grows with its partial sums: for output (pixel, channel) with the energy of
    the pixel's input patch times the channel's weight norm, and it shows most at the outputs of
    largest magnitude, which sit in a few channels.  A handful of random pixels sees neither tail (a
    correct f32 sum in another order then needed 2.1 e_seq, tests/test_layer_ref.py), so a third of
    the pixels are those of largest patch energy, for which the norm over the channels of the ideal is
    the free estimate (every channel's worst pixels at once), a third those holding the largest
    |ideal|, a third random.  As many pixels as the layer's K lets a test afford: 384 for a 1x1 (the
    heads' 57 channels), 96 for a 3x3 or 7x7.  A pure function of the ideal: the code under test has
    no part in it."""
    P = ideal_values.shape[0]
    n = min({1: 384, 3: 96, 7: 96}[ksize], P)
    third = (n + 2) // 3
    energy = np.argsort(-np.linalg.norm(ideal_values, axis=1), kind="stable")[:third]
    peak = np.argsort(-np.abs(ideal_values).max(axis=1), kind="stable")[:third]
    top = np.unique(np.concatenate([energy, peak]))
    rest = np.setdiff1d(np.arange(P), top)
    extra = rng.choice(rest, min(max(n - len(top), 0), len(rest)), replace=False) if len(rest) else rest
    return np.concatenate([top, extra]).astype(np.int64)


def tolerance(ideal_values, e_seq, precision):
    """2 e_seq + r |ideal|: r = 2^-17 where the output is split-stored (bf16x3), 2^-23 for plain f32."""
    r = R_SPLIT if precision == "bf16x3" else R_F32
    return 2.0 * e_seq + r * np.abs(ideal_values)
