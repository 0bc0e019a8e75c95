"""Helpers of tests/test_gpu_layerwise.py (a plain module: no fixtures, no collection hooks): the
configurations, the checked pixels, and the comparison of one probe point with oracle/layer_ref.py."""
import numpy as np

from oracle import layer_ref as R

# name: (n, h, w), settings.  frames: the (first, count) frame ranges that are extracted and checked
# (default: all).  The settings a configuration does not name are the defaults: algo 4, chunk-planar
# stage tensors, fused heads, split-K allowed.
CONFIGS = {
    # maps 5 x 49, 10 x 98, 20 x 196: one column past a 48- and a 16-wide tile, one row past a 4-row tile
    "1x40x392": dict(shape=(1, 40, 392)),
    # maps 5 x 7 and 17 x 17: multi-frame small-launch 7x7 kernels
    "3x40x56": dict(shape=(3, 40, 56)),
    "2x136x136": dict(shape=(2, 136, 136)),
    # maps 23 x 29 = 667 px per frame: raster tiles cross the frame borders at three offsets
    "3x184x232": dict(shape=(3, 184, 232)),
    "3x184x232-batch_invariant": dict(shape=(3, 184, 232), batch_invariant=True),
    # maps 5 x 46, 10 x 92, 20 x 184 on 4 x 48 tiles ragged in rows and columns; 256 frames give conv4_3
    # and conv5_1..3 (2 x 2 x 256 workgroups) the 1024 workgroups of the register-weight kernels
    "256x40x368": dict(shape=(256, 40, 368), frames=((0, 2), (254, 2))),
    "2x64x80-algo0": dict(shape=(2, 64, 80), algo=0),
    "2x64x80-algo3": dict(shape=(2, 64, 80), algo=3),
    "2x64x80-algo4": dict(shape=(2, 64, 80), algo=4),
    "2x64x80-algo5": dict(shape=(2, 64, 80), algo=5),
    "2x64x80-pixel_major": dict(shape=(2, 64, 80), planar=False),
    "2x64x80-heads_unfused": dict(shape=(2, 64, 80), head_fused=False),
}
PRECISIONS = ("bf16x3", "fp32")


def network_input(shape):
    n, h, w = shape
    return np.random.default_rng(n * 1000003 + h * 1009 + w).uniform(-0.5, 0.5, (n, 3, h, w)).astype(np.float32)


def apply(ctx, cfg, precision, monkeypatch):
    """Put the context into the configuration (every setting, so the order of the tests does not matter)."""
    ctx.set_precision(precision)
    ctx.set_conv_algo(cfg.get("algo", 4))
    ctx.set_stage_layout(cfg.get("planar", True))
    ctx.set_batch_invariant(cfg.get("batch_invariant", False))
    if cfg.get("head_fused", True):
        monkeypatch.delenv("OP_HEAD_FUSED", raising=False)
    else:
        monkeypatch.setenv("OP_HEAD_FUSED", "0")  # read per forward


def conv11_mode(cfg):
    """Which conv1_1 the bf16x3 forward runs: conv1_pair.hip's split-product MFMA form under the conv_big
    families (algo 4, 5), conv11.hip's f32 FMAs otherwise (forward.hip run_forward)."""
    return "mfma" if cfg.get("algo", 4) in (4, 5) else "f32"


def frame_ranges(cfg):
    return cfg.get("frames", ((0, cfg["shape"][0]),))


def probe(ctx, x, cfg, point):
    """The point's tensor for the configuration's frame ranges, concatenated."""
    return np.concatenate([ctx.forward_probe(x, point, frames=fr) for fr in frame_ranges(cfg)], axis=0)


def checked_pixels(n_batch, frames, h, w, rng):
    """(P, 3) pixels (frame, y, x) of `frames` extracted h x w maps of an n_batch-frame launch: all of
    them when the launch has <= 4096 pixels; else every row and column among the first and last 4 or
    within 1 of a multiple of 4 (hence of 8, 16, 32 and 48: the tile edges of every kernel), which
    includes the last row of each frame and the first row of the next (raster tiles cross frames),
    and 256 random pixels."""
    if n_batch * h * w <= 4096:
        return R.all_pixels(frames, h, w)

    def lines(n):
        i = np.arange(n)
        return (i < 4) | (i >= n - 4) | (i % 4 != 2)

    mask = np.zeros((frames, h, w), bool)
    mask |= lines(h)[None, :, None] | lines(w)[None, None, :]
    k = min(256, mask.size)
    mask.reshape(-1)[rng.choice(mask.size, k, replace=False)] = True
    f, y, x = np.nonzero(mask)
    return np.stack([f, y, x], axis=1).astype(np.int64)


def compare(point, precision, conv11, weights, inp, out, n_batch, net="posenet", inp_hi=None):
    """One probe point against its reference.  inp / out: the probed input and output tensors (the
    first 57 channels of a map point; net "facenet" / "handnet": the first C, tests/cpm_layerwise.py;
    inp_hi: the hi halves of the input's stored pairs, layer_ref.ideal's inputs_hi).  -> dict(max_err, e_seq, ratio = max |err| / e_seq, need = the
    factor on e_seq the point needs once the output rounding r |ideal| is taken off (the test allows
    2), worst = the largest |err| / tolerance with its (frame, channel, y, x), n = outputs checked)."""
    frames, ch, h, w = out.shape
    rng = np.random.default_rng(point)
    pix = checked_pixels(n_batch, frames, h, w, rng)
    want = R.ideal(point, precision, inp, weights, pix, conv11, net=net, inputs_hi=inp_hi)
    assert want.shape == (len(pix), ch), (want.shape, out.shape)
    sample = R.yardstick_pixels(want, weights[R.point_spec(point, net)[1][-1][0][0][0]][0].shape[2], rng)
    seq = R.seq_f32(point, precision, inp, weights, pix[sample], conv11, net=net, inputs_hi=inp_hi)
    e_seq = float(np.abs(seq - want[sample]).max())
    got = out[pix[:, 0], :, pix[:, 1], pix[:, 2]].astype(np.float64)
    err = np.abs(got - want)
    tol = R.tolerance(want, e_seq, precision)
    rel = err / np.maximum(tol, 1e-300)
    need = float(((err - (tol - 2.0 * e_seq)) / e_seq).max()) if e_seq > 0 else float("inf")
    i, c = np.unravel_index(int(np.argmax(rel)), rel.shape)
    return dict(max_err=float(err.max()), e_seq=e_seq, ratio=float(err.max() / e_seq) if e_seq > 0 else float("inf"),
                need=need, worst=float(rel[i, c]), at=(int(pix[i, 0]), int(c), int(pix[i, 1]), int(pix[i, 2])),
                got=float(got[i, c]), want=float(want[i, c]), n=int(err.size), bad=int((err > tol).sum()))
