"""Helpers of tests/test_gpu_cpm_layerwise.py (a plain module: no fixtures, no collection hooks): the
configurations of the FaceNet / HandNet layer-wise check and the comparison of one probe point of
op_cpm_forward_probe with oracle/layer_ref.py (net="facenet" / "handnet").

What the CPM plan (csrc/cpm.hip cpm_run) asks of the shared conv kernels, and which configuration is
there for it.  The census names are those of _lib.conv_census; "7x7" are the 25 Mconv1..5 launches,
"3x3" the 11 of conv2_1 .. conv5_3_CPM without the two fused conv + pool launches (3x3_pool).

* Mconv1 has 13 chunks in FaceNet (odd) and 10 in HandNet; Mconv2..5 have 8.
  - conv_m16q (7x7_q: split-K allowed, <= 4800 map pixels) declines an odd chunk count
    (launch_conv_m16q: ``s.c16 & 1``), so FaceNet's Mconv1 runs conv_m16 (census ``npx``) where the
    raster tiling fits, i.e. maps of >= 640 pixels, and the conv_big fallback (7x7_other) on smaller
    maps; 13 is prime, so no split-K candidate divides it and Mconv1 never splits.  HandNet's Mconv1
    runs conv_m16q with 5 chunk pairs x 2 tap ranges, Mconv2..5 with 4 x 2.
  - without split-K (batch-invariant) all 25 run conv_m16 (>= 640 px) or conv_big (smaller).
* 3x3: conv_m16k on 4 x 48 tiles (3x3_w48) or 8 x 32 tiles (3x3_w32), conv_big (3x3_big) on maps
  too narrow for either, split-K (3x3_splitk) when the launch has few workgroups.

name: shape (n, h, w) and settings; what is not named is the default: split-K allowed, fused heads.
frames: the (first, count) frame ranges that are extracted and checked (default: all)."""
import numpy as np

import layerwise as LW
from oracle import layer_ref as R

ARCHS = ("facenet", "handnet")
CONFIGS = {
    # maps 5 x 7, one frame: the smallest launches.  7x7: FaceNet Mconv1 on conv_big (7x7_other 5), the
    # rest on conv_m16q; 3x3 all on conv_big (3x3_big 11), the fused pools with split-K
    "1x40x56": dict(shape=(1, 40, 56)),
    # several frames at the smallest maps: tiles that hold more than one whole frame
    "3x40x56": dict(shape=(3, 40, 56)),
    # maps 17 x 17 (68 x 68, 34 x 34): conv3_x on 4 x 48 tiles (3x3_w48 4), the /8 layers on conv_big
    "2x136x136": dict(shape=(2, 136, 136)),
    # maps 5 x 49, 10 x 98, 20 x 196: one column past a 48- and a 16-wide tile, one row past a 4-row tile
    "1x40x392": dict(shape=(1, 40, 392)),
    # maps 23 x 29 = 667 px per frame, 2001 in all: every 3x3 on 8 x 32 tiles (3x3_w32 11); FaceNet's
    # Mconv1 on conv_m16 raster tiles (npx 2) that cross the frame borders, the rest on conv_m16q
    "3x184x232": dict(shape=(3, 184, 232)),
    # the same without split-K: all 25 7x7 on conv_m16 (npx 2: 25), no 3x3_splitk
    "3x184x232-batch_invariant": dict(shape=(3, 184, 232), batch_invariant=True),
    # OP_HEAD_FUSED=0: conv6_1 + conv6_2 and Mconv6 + Mconv7 as two launches each
    "2x64x80-heads_unfused": dict(shape=(2, 64, 80), head_fused=False),
    # ---- the product's dispatch: the detectors run 368 x 368 crops, one (op_cpm_detect) or a batch
    # (op_cpm_detect_batch; n = 4 stands for it) ----
    # n = 1 at 368 x 368 (maps 184, 92, 46 wide): conv2_1 on 8 x 32 tiles (184 x 184: both tile shapes
    # use 95.8 % of the lanes and the tie goes to 4 x 48 only below 128 columns), the other ten 3x3 on
    # 4 x 48 tiles, all 13 conv_m16k launches with split-K (the "46-wide layers" rule of launch_m16k:
    # at most 138 workgroups each); FaceNet's Mconv1 on conv_m16 with npx 2, tight pitch, unsplit; the
    # other 7x7 on conv_m16q.  None of this depends on the rows beyond: h / 2 a multiple of 8 (conv2_1's
    # tie) and h / 8 * 46 >= 640 map pixels (conv_m16's raster tiling), so 112 x 368 (maps 14 x 46)
    # is the smallest frame with the same census; test_product_dispatch_census asserts the equality
    "1x112x368": dict(shape=(1, 112, 368)),
    "1x112x368-batch_invariant": dict(shape=(1, 112, 368), batch_invariant=True),
    # n = 4 at 368 x 368: 8464 map pixels are past conv_m16q's 4800, so Mconv2..5 (and HandNet's
    # Mconv1, S = 2: the only candidate dividing 10 chunks) run conv_m16 with npx 5 and split-K chosen
    # jointly from the workgroup count (launch_conv_big, "Split-K"), Mconv1 npx 2; of the 3x3 only
    # the seven /8 launches (192 workgroups each) still split.  Those choices are keyed on the number
    # of workgroups, i.e. on the batch's pixel count: 4 x 240 x 368 and 8 x 112 x 368 (61 - 65 % of the
    # pixels) take npx 3 and split eleven 3x3 launches instead.  No smaller shape has this census, so
    # the shape itself, checked at checked_pixels' edge-plus-random sample of the last frame: the one
    # whose first rows end a raster tile begun in the frame before and whose last rows are the
    # batch's partial tile (the rows that begin such a tile are checked in every frame of 3x184x232);
    # one frame keeps point 1's float64 work (184 x 184 pixels x 4 pooled positions) at that of
    # 3x184x232
    "4x368x368": dict(shape=(4, 368, 368), frames=((3, 1),)),
}
# (small configuration, the 368 x 368 launch whose census it must equal)
PRODUCT_DISPATCH = (("1x112x368", (1, 368, 368)), ("1x112x368-batch_invariant", (1, 368, 368)))


def network_input(shape):
    return LW.network_input(shape)


def apply(ctx, cfg, monkeypatch):
    """Put the context into the configuration (every setting, so the order of the tests does not matter)."""
    ctx.set_batch_invariant(cfg.get("batch_invariant", False))
    if cfg.get("head_fused", True):
        monkeypatch.delenv("OP_HEAD_FUSED", raising=False)
    else:
        monkeypatch.setenv("OP_HEAD_FUSED", "0")  # read per pair launch (csrc/cpm.hip cpair)


def probe(ctx, x, cfg, point, hi=False):
    """The point's tensor (hi: the hi halves of its stored pairs) for the configuration's frame
    ranges, concatenated."""
    return np.concatenate([ctx.forward_probe(x, point, frames=fr, hi=hi) for fr in LW.frame_ranges(cfg)], axis=0)


def compare(arch, point, weights, inp, inp_hi, out, n_batch):
    """One probe point against its reference (layerwise.compare: the same pixels, yardstick and
    tolerance 2 e_seq + 2^-17 |ideal|).  inp: the probed input tensor, a map point's whole [heat |
    pad | feature], inp_hi the hi halves of its stored pairs; out: the probed output, the first C
    channels of a map point.  The CPM nets run in bf16x3 with the MFMA conv1_1 of conv1_pair.hip.
    Why the hi halves: 0.1 % of the stored values hi + lo lie exactly halfway between two bf16 values,
    and the sum does not say whether the kernel stored (lower, +half a step) or (upper, -half).  The
    reading layer's products w_hi x_hi + w_hi x_lo + w_lo x_hi differ between the two by w_lo times a
    bf16 step of x; the ideal from split(hi + lo) then missed the GPU by up to 2.5 e_seq at an output
    whose input pixel held such a value (handnet 4x368x368 point 45)."""
    return LW.compare(point, "bf16x3", "mfma", weights, inp, out, n_batch, net=arch, inp_hi=inp_hi)
