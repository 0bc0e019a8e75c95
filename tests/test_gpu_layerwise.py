"""Every launch of the forward held to its own reference (op_forward_probe, oracle/layer_ref.py).

For a configuration and each probe point p >= 1 the point's input and output are read back from the
GPU and the output is compared, elementwise over all channels at the checked pixels, with the float64
ideal of that one layer (or fused group) applied to the input the GPU gave it:

    |y_gpu - ideal| <= 2 e_seq + r |ideal|

e_seq = the largest |seq_f32 - ideal| over the layer's sampled pixels (the same terms accumulated in
f32 one at a time), r = 2^-17 for split-stored outputs (bf16x3) and 2^-23 for f32.  The MFMA chain
sums 16- or 32-product groups before it adds to the accumulator, so it can be as bad as the
sequential order or better; split-K adds one more f32 association: hence the factor 2.  (The exact
path's v_mfma_f32_32x32x2_f32 sums two products per step: measured, its error has the r.m.s. of the
sequential sum in the kernel's channel order, so there the factor covers only what the sampled
pixels miss of the tail; layer_ref.yardstick_pixels says how they are chosen.)  The tolerance comes
to 0.5e-5 .. 3e-5 + 8e-6 |y| in bf16x3; tests/test_layer_ref.py shows that one lost (tap, 16-channel
chunk) at one pixel, or a lost cross product, misses it by 100x and more.

The configurations (tests/layerwise.py) are the smallest shapes that reach each dispatch branch of
conv_big.hip; each prints its conv_census, and every point prints max |err|, e_seq and their ratio
(DESIGN.md §2 has the table)."""
import ctypes

import numpy as np
import pytest

import layerwise as LW
from conftest import pkg_module
from oracle import layer_ref as R

pytestmark = pytest.mark.gpu

CASES = [(c, p) for c in LW.CONFIGS for p in LW.PRECISIONS]


@pytest.fixture(scope="module")
def lib():
    return pkg_module("_lib")


@pytest.fixture(scope="module")
def lctx(lib, rand_weights):
    c = lib.Context(0)
    c.set_weights(rand_weights)
    yield c
    c.close()


_inputs = {}
_probed = {"key": None}


def _x(shape):
    if shape not in _inputs:
        _inputs[shape] = LW.network_input(shape)
    return _inputs[shape]


def _probe(ctx, x, name, precision, point):
    """Probes of the current configuration, kept while it is the current one (a point's output is the
    next point's input; the forward is deterministic run to run)."""
    if _probed["key"] != (name, precision):
        _probed.clear()
        _probed["key"] = (name, precision)
    if point not in _probed:
        _probed[point] = LW.probe(ctx, x, LW.CONFIGS[name], point)
    return _probed[point]


@pytest.mark.parametrize("point", range(1, R.N_POINTS))
@pytest.mark.parametrize("name,precision", CASES)
def test_point_vs_single_layer_reference(lib, lctx, rand_weights, monkeypatch, name, precision, point):
    cfg = LW.CONFIGS[name]
    LW.apply(lctx, cfg, precision, monkeypatch)
    x = _x(cfg["shape"])
    src = R.point_spec(point)[0]
    inp = _probe(lctx, x, name, precision, src)
    out = _probe(lctx, x, name, precision, point)
    info = lib.probe_table()[point]
    assert out.shape[1] == info[1] and out.shape[2:] == (x.shape[2] // info[2], x.shape[3] // info[2]), out.shape
    if point in R.MAP_POINTS:
        # the feature slice of the buffer the next Mconv1 reads is conv4_4_CPM's output, bit for bit
        # (the copy into the chunk-planar tensor when the stages run on it)
        assert np.array_equal(out[:, 57:], _probe(lctx, x, name, precision, 11))
        out = out[:, :57]
    assert out.shape[1] == R.out_channels(point, rand_weights)
    r = LW.compare(point, precision, LW.conv11_mode(cfg), rand_weights, inp, out, x.shape[0])
    print("LAYERWISE %s %s point %d %s: max|err| %.3e e_seq %.3e ratio %.2f need %.2f worst err/tol %.3f at %s (%d outputs)" % (
        name, precision, point, info[0], r["max_err"], r["e_seq"], r["ratio"], r["need"], r["worst"], r["at"], r["n"]))
    assert r["bad"] == 0, r


@pytest.mark.parametrize("name,precision", CASES)
def test_census_of_the_configuration(lib, lctx, monkeypatch, name, precision):
    """Which kernels the configuration's forward ran (printed; the kernel coverage of this file).
    launch_conv_m16r takes a 3x3 launch from 1024 workgroups of 4 x 48 tiles = groups x (Co / 128) x n
    x tiles.  On 40 x 368 frames (20, 6 and 2 tiles per frame at /2, /4, /8) 128 frames reach that for
    conv2_1 .. conv4_2 only (measured: 3x3_r128 6 + 3x3_r_pool 2); conv4_3 and conv5_1 .. conv5_3 have
    2 x 2 x n workgroups and need 256 frames, the smallest batch at which every 3x3 launch from conv2_1
    to conv5_3 except conv4_4 (1 x 2 x n) runs conv_m16r: 10 + the 2 pooled launches."""
    cfg = LW.CONFIGS[name]
    LW.apply(lctx, cfg, precision, monkeypatch)
    x = _x(cfg["shape"])
    lib.conv_census(reset=True)
    lctx.forward(x)
    cen = lib.conv_census(reset=True)
    print("CENSUS %s %s: %s" % (name, precision, {k: v for k, v in cen.items() if v}))
    if name == "256x40x368" and precision == "bf16x3":
        assert cen["3x3_r128"] + cen["3x3_r_pool"] >= 10, cen


# ---- the probe itself ----
@pytest.mark.parametrize("precision", LW.PRECISIONS)
def test_point_0_is_the_network_input(lctx, monkeypatch, precision):
    cfg = LW.CONFIGS["3x40x56"]
    LW.apply(lctx, cfg, precision, monkeypatch)
    x = _x(cfg["shape"])
    got = lctx.forward_probe(x, 0)
    assert np.array_equal(got, x if precision == "fp32" else R.recon(x))
    one = lctx.forward_probe(x, 0, frames=(2, 1))
    assert np.array_equal(one, got[2:3])


@pytest.mark.parametrize("name", ["3x40x56", "2x64x80-pixel_major", "2x64x80-heads_unfused", "2x64x80-algo0"])
@pytest.mark.parametrize("precision", LW.PRECISIONS)
def test_map_points_are_the_stage_maps(lctx, monkeypatch, name, precision):
    """Every map point's first 57 channels are forward_stages()'s (paf, heat) of that stage, and point
    45's are forward()'s: as stored, i.e. through the hi/lo split in bf16x3 (the dense f32 copy the
    maps come from is written before the split store), bit for bit in fp32."""
    cfg = LW.CONFIGS[name]
    LW.apply(lctx, cfg, precision, monkeypatch)
    x = _x(cfg["shape"])
    stored = R.recon if precision == "bf16x3" else (lambda a: a)
    pafs, heats = lctx.forward_stages(x)
    for s, point in enumerate(R.MAP_POINTS):
        got = lctx.forward_probe(x, point)
        assert np.array_equal(got[:, :38], stored(pafs[s])), (s, point)
        assert np.array_equal(got[:, 38:57], stored(heats[s])), (s, point)
    paf, heat = lctx.forward(x)
    last = lctx.forward_probe(x, 45)
    assert np.array_equal(last[:, :38], stored(paf)) and np.array_equal(last[:, 38:57], stored(heat))


@pytest.mark.parametrize("precision", LW.PRECISIONS)
def test_probe_does_not_disturb_the_next_forward(lctx, monkeypatch, precision):
    cfg = LW.CONFIGS["3x40x56"]
    LW.apply(lctx, cfg, precision, monkeypatch)
    x = _x(cfg["shape"])
    want = lctx.forward(x)
    for point in (20, 3, 45, 17):  # stops inside the joined Mconv2..5 run, a pooled point, the end
        lctx.forward_probe(x, point, frames=(1, 2))
        got = lctx.forward(x)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), point


def test_bad_arguments_are_refused(lib, lctx, monkeypatch):
    LW.apply(lctx, LW.CONFIGS["3x40x56"], "bf16x3", monkeypatch)
    x = _x((3, 40, 56))
    L = lib.lib()
    out = np.empty((3, 256, 5, 7), np.float32)

    def call(point, f0, nf, floats, xp=lib.ptr(x), op=lib.ptr(out), h=40, w=56):
        return L.op_forward_probe(lctx.h, xp, 3, h, w, point, f0, nf, op, floats)

    assert call(13, 0, 3, out.size) == lib.OP_OK
    for bad in ((-1, 0, 3, out.size), (46, 0, 3, out.size), (13, -1, 3, out.size), (13, 0, 0, 0), (13, 1, 3, out.size),
                (13, 3, 1, out.size // 3), (13, 0, 3, out.size - 1), (13, 0, 3, out.size + 1), (13, 0, 2, out.size),
                (13, 2 ** 31 - 1, 2, out.size // 3 * 2)):
        assert call(*bad) == lib.OP_ERR_INVALID, bad
        assert lib.last_error()
    assert call(13, 0, 3, out.size, xp=None) == lib.OP_ERR_INVALID
    assert call(13, 0, 3, out.size, op=None) == lib.OP_ERR_INVALID
    assert call(13, 0, 3, out.size, h=44) == lib.OP_ERR_INVALID
    name, ch, div = ctypes.c_char_p(), ctypes.c_int32(), ctypes.c_int32()
    for point in (-1, 46):
        assert L.op_forward_probe_info(point, ctypes.byref(name), ctypes.byref(ch), ctypes.byref(div)) == lib.OP_ERR_INVALID
    with pytest.raises(ValueError):
        lctx.forward_probe(x, 13, frames=(2, 2))
    table = lib.probe_table()
    assert len(table) == R.N_POINTS and table[0] == ("input", 3, 1) and table[45] == ("stage6", 185, 8)
    assert [i for i, t in enumerate(table) if t[1] == 185] == list(R.MAP_POINTS)
