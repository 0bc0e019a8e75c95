"""Every launch of the FaceNet / HandNet forward held to its own reference (op_cpm_forward_probe,
oracle/layer_ref.py with net="facenet" / "handnet").

As tests/test_gpu_layerwise.py does for CocoPoseNet: for a net, a configuration and each probe point
p >= 1 the point's input and output are read back from the GPU and the output is compared,
elementwise over all channels at the checked pixels, with the float64 ideal of that one layer (or
pair, or conv + pool) applied to the input the GPU gave it:

    |y_gpu - ideal| <= 2 e_seq + 2^-17 |ideal|

e_seq = the largest |seq_f32 - ideal| over the layer's sampled pixels: the same terms accumulated in
f32 one at a time in the kernels' physical chunk order (for Mconv1: feature chunks 0..7, then the heat
chunks).  tests/test_layer_ref.py shows what misses it: one lost (tap, chunk) in FaceNet's 13th
chunk, a lost cross product there, Mconv1's weights in logical order, an off-by-one heat slice, a
dropped split-K half.

The configurations (tests/cpm_layerwise.py) are the smallest shapes that reach each dispatch branch
the CPM plan takes, the product's 368 x 368 launches included; each prints its conv_census, and every
point prints max |err|, e_seq, their ratio and the factor on e_seq it needed (DESIGN.md §2a has the
table)."""
import ctypes

import numpy as np
import pytest

import cpm_layerwise as CL
from conftest import pkg_module
from oracle import layer_ref as R

pytestmark = pytest.mark.gpu

CASES = [(a, c) for a in CL.ARCHS for c in CL.CONFIGS]


@pytest.fixture(scope="module")
def lib():
    return pkg_module("_lib")


_nets = {}


@pytest.fixture(scope="module")
def nets(lib):
    """{arch: (CpmContext, weights)}, made on first use and closed with the module."""
    def get(arch):
        if arch not in _nets:
            W = pkg_module("weights").random_weights(seed=4, arch=arch)
            c = lib.CpmContext(arch, 0)
            c.set_weights(W)
            _nets[arch] = (c, W)
        return _nets[arch]
    yield get
    for c, _ in _nets.values():
        c.close()
    _nets.clear()


_inputs = {}
_probed = {"key": None}


def _x(shape):
    if shape not in _inputs:
        _inputs[shape] = CL.network_input(shape)
    return _inputs[shape]


def _probe(ctx, x, arch, name, point, hi=False):
    """Probes of the current (net, configuration), kept while it is the current one (a point's output
    is the next point's input; the forward is deterministic run to run).  hi: the hi halves."""
    if _probed["key"] != (arch, name):
        _probed.clear()
        _probed["key"] = (arch, name)
    if (point, hi) not in _probed:
        _probed[point, hi] = CL.probe(ctx, x, CL.CONFIGS[name], point, hi)
    return _probed[point, hi]


@pytest.mark.parametrize("point", range(1, R.N_POINTS))
@pytest.mark.parametrize("arch,name", CASES)
def test_point_vs_single_layer_reference(lib, nets, monkeypatch, arch, name, point):
    """The ideal is formed from the input's stored pairs (its hi halves are probed as well):
    tests/cpm_layerwise.compare says what hi + lo alone cost at one output of 45012."""
    ctx, W = nets(arch)
    cfg = CL.CONFIGS[name]
    CL.apply(ctx, cfg, monkeypatch)
    x = _x(cfg["shape"])
    C, heat = R.CPM_MAPS[arch], R.cpm_heat_channels(arch)
    src = R.point_spec(point, arch)[0]
    inp = _probe(ctx, x, arch, name, src)
    inp_hi = _probe(ctx, x, arch, name, src, hi=True)
    assert np.array_equal(R.bf16_rne(inp_hi), inp_hi) and np.array_equal(R.bf16_rne(inp - inp_hi), inp - inp_hi)
    out = _probe(ctx, x, arch, name, point)
    info = lib.cpm_probe_table(arch)[point]
    assert out.shape[1] == info[1] and out.shape[2:] == (x.shape[2] // info[2], x.shape[3] // info[2]), out.shape
    if point in R.MAP_POINTS:
        # the pair writes its heat slice of the buffer it has just read the feature from (stage 1) or
        # that the next Mconv1 reads: the channels behind the C maps stay exactly zero (zero weights and
        # bias up to the 8-multiple stored, the arena's memset beyond), and the feature slice is still
        # conv5_3_CPM's output bit for bit
        assert out.shape[1] == heat + 128
        assert not out[:, C:heat].any()
        assert np.array_equal(out[:, heat:], _probe(ctx, x, arch, name, R.CPM_FEATURE_POINT))
        out = out[:, :C]
    assert out.shape[1] == R.out_channels(point, W, arch)
    r = CL.compare(arch, point, W, inp, inp_hi, out, x.shape[0])
    print("CPM-LAYERWISE %s %s point %d %s: max|err| %.3e e_seq %.3e ratio %.2f need %.2f worst err/tol %.3f at %s (%d outputs)" % (
        arch, name, point, info[0], r["max_err"], r["e_seq"], r["ratio"], r["need"], r["worst"], r["at"], r["n"]))
    assert r["bad"] == 0, r


def _census(lib, ctx, x):
    lib.conv_census(reset=True)
    ctx.forward(x)
    cen = lib.conv_census(reset=True)
    return {k: v for k, v in cen.items() if v}


@pytest.mark.parametrize("arch,name", CASES)
def test_census_of_the_configuration(lib, nets, monkeypatch, arch, name):
    """Which kernels the configuration's forward ran (printed; the kernel coverage of this file), and
    the branches tests/cpm_layerwise.py says the configuration is there for."""
    ctx, _ = nets(arch)
    cfg = CL.CONFIGS[name]
    CL.apply(ctx, cfg, monkeypatch)
    cen = _census(lib, ctx, _x(cfg["shape"]))
    print("CPM-CENSUS %s %s: %s" % (arch, name, cen))
    npx = cen.get("npx", {})
    assert cen["conv1_pair"] == 1 and cen["3x3_pool"] == 2
    assert sum(npx.values()) + cen.get("7x7_q", 0) + cen.get("7x7_other", 0) == 25
    assert cen.get("3x3_w48", 0) + cen.get("3x3_w32", 0) + cen.get("3x3_big", 0) == 11
    if cfg.get("batch_invariant"):
        assert not cen.get("7x7_splitk") and not cen.get("3x3_splitk") and not cen.get("7x7_q")
    elif arch == "facenet":  # 13 chunks: never conv_m16q, never split
        assert cen.get("7x7_q", 0) <= 20 and cen.get("7x7_splitk", 0) <= 20
    if name == "3x184x232":
        assert cen["3x3_w32"] == 11 and (npx == {2: 5} if arch == "facenet" else cen["7x7_q"] == 25)
    if name == "3x184x232-batch_invariant":
        assert npx == {2: 25}
    if name == "1x40x56":
        assert cen["3x3_big"] == 11 and cen.get("7x7_other", 0) == (5 if arch == "facenet" else 0)
    if name == "4x368x368":
        assert npx == {2: 5, 5: 20} and "7x7_q" not in cen and cen["3x3_splitk"] == 7
        assert cen["7x7_splitk"] == (20 if arch == "facenet" else 25)


@pytest.mark.parametrize("small,full", CL.PRODUCT_DISPATCH)
@pytest.mark.parametrize("arch", CL.ARCHS)
def test_product_dispatch_census(lib, nets, monkeypatch, arch, small, full):
    """The small configuration that stands for one 368 x 368 crop runs the same kernels, launch for
    launch of the census, as the crop itself (tests/cpm_layerwise.py has the derivation)."""
    ctx, _ = nets(arch)
    cfg = CL.CONFIGS[small]
    CL.apply(ctx, cfg, monkeypatch)
    got = _census(lib, ctx, _x(cfg["shape"]))
    want = _census(lib, ctx, _x(full))
    print("CPM-CENSUS %s %s: %s == %dx%dx%d: %s" % ((arch, small, got) + full + (want,)))
    assert got == want


# ---- the probe itself ----
@pytest.mark.parametrize("arch", CL.ARCHS)
def test_point_0_is_the_network_input(nets, monkeypatch, arch):
    ctx, _ = nets(arch)
    cfg = CL.CONFIGS["3x40x56"]
    CL.apply(ctx, cfg, monkeypatch)
    x = _x(cfg["shape"])
    got = ctx.forward_probe(x, 0)
    assert np.array_equal(got, R.recon(x))
    one = ctx.forward_probe(x, 0, frames=(2, 1))
    assert np.array_equal(one, got[2:3])


@pytest.mark.parametrize("name", ["1x40x56", "3x40x56", "2x64x80-heads_unfused", "3x184x232"])
@pytest.mark.parametrize("arch", CL.ARCHS)
def test_last_map_point_is_the_forward_output(nets, monkeypatch, arch, name):
    """Point 45's first C channels are op_cpm_forward's maps as stored.  The last pair's epilogue
    (conv_head.hip's fused kernel; conv_bf16x3.hip store_tile for the two-launch form) writes the dense
    f32 copy and the hi/lo split from the same f32 value v = acc + bias, so recon(forward) == point 45
    bit for bit."""
    ctx, _ = nets(arch)
    cfg = CL.CONFIGS[name]
    CL.apply(ctx, cfg, monkeypatch)
    x = _x(cfg["shape"])
    C = R.CPM_MAPS[arch]
    maps = ctx.forward(x)
    last = ctx.forward_probe(x, 45)
    assert maps.shape[1] == C and np.array_equal(last[:, :C], R.recon(maps))


@pytest.mark.parametrize("arch", CL.ARCHS)
def test_probe_does_not_disturb_the_next_forward(nets, monkeypatch, arch):
    ctx, _ = nets(arch)
    cfg = CL.CONFIGS["3x40x56"]
    CL.apply(ctx, cfg, monkeypatch)
    x = _x(cfg["shape"])
    want = ctx.forward(x)
    for point in (5, 20, 45):  # inside the ping-ponged conv3 and Mconv runs, the end
        ctx.forward_probe(x, point, frames=(1, 2))
    assert np.array_equal(ctx.forward(x), want)
    for point in (5, 20, 45):
        ctx.forward_probe(x, point)
        assert np.array_equal(ctx.forward(x), want), point


def test_bad_arguments_are_refused(lib, nets, monkeypatch):
    ctx, _ = nets("handnet")
    CL.apply(ctx, CL.CONFIGS["3x40x56"], monkeypatch)
    x = _x((3, 40, 56))
    L = lib.lib()
    out = np.empty((3, 512, 5, 7), np.float32)

    def call(point, f0, nf, floats, xp=lib.ptr(x), op=lib.ptr(out), h=40, w=56, c=ctx.h):
        return L.op_cpm_forward_probe(c, xp, 3, h, w, point, f0, nf, op, floats)

    assert call(13, 0, 3, out.size) == lib.OP_OK
    full = out.copy()
    assert call(lib.CPM_PROBE_HI + 13, 0, 3, out.size) == lib.OP_OK  # the hi halves of the same pairs
    assert np.array_equal(R.bf16_rne(out), out) and np.array_equal(R.bf16_rne(full - out), full - out)
    assert np.abs(full - out).max() > 0
    for bad in (lib.CPM_PROBE_HI - 1, lib.CPM_PROBE_HI + 46, 2 * lib.CPM_PROBE_HI + 13):
        assert call(bad, 0, 3, out.size) == lib.OP_ERR_INVALID, bad
    for bad in ((-1, 0, 3, out.size), (46, 0, 3, out.size), (13, -1, 3, out.size), (13, 0, 0, 0), (13, 1, 3, out.size),
                (13, 3, 1, out.size // 3), (13, 0, 3, out.size - 1), (13, 0, 3, out.size + 1), (13, 0, 2, out.size),
                (13, 2 ** 31 - 1, 2, out.size // 3 * 2)):
        assert call(*bad) == lib.OP_ERR_INVALID, bad
        assert lib.last_error()
    assert call(13, 0, 3, out.size, xp=None) == lib.OP_ERR_INVALID
    assert call(13, 0, 3, out.size, op=None) == lib.OP_ERR_INVALID
    assert call(13, 0, 3, out.size, h=44) == lib.OP_ERR_INVALID
    assert call(13, 0, 3, out.size, c=None) == lib.OP_ERR_INVALID
    name, ch, div = ctypes.c_char_p(), ctypes.c_int32(), ctypes.c_int32()
    for arch, point in ((2, -1), (2, 46), (0, 13), (3, 13)):
        assert L.op_cpm_probe_info(arch, point, ctypes.byref(name), ctypes.byref(ch), ctypes.byref(div)) == lib.OP_ERR_INVALID
    with pytest.raises(ValueError):
        ctx.forward_probe(x, 13, frames=(2, 2))
    bare = lib.CpmContext("handnet", 0)  # no weights: a state error, not a launch
    try:
        assert call(13, 0, 3, out.size, c=bare.h) == lib.OP_ERR_STATE
    finally:
        bare.close()
    for arch, heat in (("facenet", 80), ("handnet", 32)):
        table = lib.cpm_probe_table(arch)
        assert len(table) == R.N_POINTS and table[0] == ("input", 3, 1) and table[45] == ("stage6", heat + 128, 8)
        assert [i for i, t in enumerate(table) if t[1] == heat + 128] == list(R.MAP_POINTS)
