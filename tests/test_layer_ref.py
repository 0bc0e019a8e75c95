"""oracle/layer_ref.py, the single-layer reference of tests/test_gpu_layerwise.py, checked on the CPU:
its fp32 ideal against the oracle's own convolution and pooling in float64, its bf16 split against
csrc/host_pack.hpp, and its tolerance against the defects it has to catch."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG_NAME, REPO
from oracle import forward as F
from oracle import layer_ref as R


def _f64_layers(weights, groups, x):
    """The groups of one step through oracle.forward in float64: concat of conv(x[:, c0:c1])."""
    out = []
    for name, c0, c1 in groups:
        W, b = weights[name]
        out.append(F.convolution_2d(x[:, c0:c1].astype(np.float64), W.astype(np.float64), b.astype(np.float64),
                                    W.shape[2] // 2))
    return np.concatenate(out, axis=1)


@pytest.mark.parametrize("point,shape", [(3, (2, 128, 6, 10)), (16, (1, 185, 5, 7))])
def test_fp32_ideal_is_the_oracle_convolution_in_float64(rand_weights, point, shape):
    """conv2_2 + ReLU + 2x2 max-pool, and the two-branch 7x7 Mconv1 of stage 2 on a map smaller than
    its kernel: layer_ref's patch gather, zero padding, channel slices and pooling against
    oracle.forward.convolution_2d / max_pooling_2d run in float64, to 1e-12."""
    rng = np.random.default_rng(point)
    x = rng.uniform(0.0, 1.0, shape).astype(np.float32)
    _, steps, pooled = R.point_spec(point)
    assert len(steps) == 1
    want = F.relu(_f64_layers(rand_weights, steps[0][0], x))
    if pooled:
        want = F.max_pooling_2d(want)
    n, _, oh, ow = want.shape
    got = R.to_nchw(R.ideal(point, "fp32", x, rand_weights, R.all_pixels(n, oh, ow)), n, oh, ow)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-12


def test_fp32_ideal_of_a_fused_head(rand_weights):
    """Point 15 (conv5_4 + conv5_5): two composed 1x1 steps with the intermediate kept in float32."""
    x = np.random.default_rng(15).uniform(0.0, 1.0, (1, 256, 3, 4)).astype(np.float32)
    _, steps, _ = R.point_spec(15)
    mid = F.relu(_f64_layers(rand_weights, steps[0][0], x)).astype(np.float32)
    want = _f64_layers(rand_weights, steps[1][0], mid)
    got = R.to_nchw(R.ideal(15, "fp32", x, rand_weights, R.all_pixels(1, 3, 4)), 1, 3, 4)
    assert got.shape == (1, 57, 3, 4) and np.abs(got - want).max() <= 1e-12


# ties (to even, both ways), a carry into the exponent, denormals, signed zeros, the largest finite
# value (rounds to inf, as host_pack.hpp does), inf, and ordinary values
_VECTOR = np.array([0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0x3F7FFFFF, 0x00000001, 0x00008000, 0x00018000,
                    0x007FFFFF, 0x80000000, 0x00000000, 0x7F7FFFFF, 0x7F800000, 0xFF800000, 0x3EAAAAAB, 0xC0490FDB,
                    0x3DCCCCCD, 0xBF000001], np.uint32)
_BF16 = np.array([0x3F80, 0x3F82, 0x3F81, 0x3F80, 0x3F80, 0x0000, 0x0000, 0x0002,
                  0x0080, 0x8000, 0x0000, 0x7F80, 0x7F80, 0xFF80, 0x3EAB, 0xC049,
                  0x3DCD, 0xBF00], np.uint32)


def test_bf16_rne_by_value():
    got = R.bf16_rne(_VECTOR.view(np.float32)).view(np.uint32)
    assert np.array_equal(got, _BF16 << 16), [hex(v) for v in got]


def test_split_matches_host_pack(tmp_path):
    """split() against csrc/host_pack.hpp's bf16_rne / bf16_f compiled with g++ (the rule pack_split
    applies to the weights), on the fixed vector and on random floats of every exponent."""
    src = tmp_path / "hp.cpp"
    src.write_text('#include "host_pack.hpp"\n'
                   'extern "C" void hp_split(const float* x, int n, float* hi, float* lo) {\n'
                   '  for (int i = 0; i < n; ++i) {\n'
                   '    hi[i] = op::bf16_f(op::bf16_rne(x[i]));\n'
                   '    lo[i] = op::bf16_f(op::bf16_rne(x[i] - hi[i]));\n'
                   '  }\n'
                   '}\n')
    so = str(tmp_path / "hp.so")
    subprocess.run(["g++", "-shared", "-fPIC", "-O1", "-std=c++17", "-I", os.path.join(REPO, PKG_NAME, "csrc"),
                    str(src), "-o", so], check=True)
    L = ctypes.CDLL(so)
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32)
    x = np.concatenate([_VECTOR, bits]).view(np.float32)
    x = np.ascontiguousarray(x[np.isfinite(x)])  # (a NaN's payload survives truncation in both; inf - inf is NaN)
    hi, lo = np.empty_like(x), np.empty_like(x)
    L.hp_split(x.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(len(x)), hi.ctypes.data_as(ctypes.c_void_p),
               lo.ctypes.data_as(ctypes.c_void_p))
    with np.errstate(invalid="ignore", over="ignore"):
        ghi, glo = R.split(x)
        ok = np.isfinite(hi)
        assert np.array_equal((ghi + glo)[ok], R.recon(x)[ok])
    assert np.array_equal(ghi.view(np.uint32), hi.view(np.uint32))
    assert np.array_equal(glo.view(np.uint32), lo.view(np.uint32))
    # the pair carries 16-17 significant bits: |x - (hi + lo)| <= 2^-17 |x| away from the denormals
    big = ok & (np.abs(x) > 1e-30)
    err = np.abs(x[big].astype(np.float64) - hi[big].astype(np.float64) - lo[big])
    assert np.all(err <= 2.0 ** -17 * np.abs(x[big]))


@pytest.fixture(scope="module")
def walked(rand_weights):
    x = np.random.default_rng(0).uniform(-0.5, 0.5, (1, 3, 64, 80)).astype(np.float32)
    return R.walk(rand_weights, x, "bf16x3", 17)


@pytest.mark.parametrize("point", [2, 9, 13, 16, 17])
def test_tolerance_does_not_hide_a_defect(rand_weights, walked, point):
    """The tolerance of tests/test_gpu_layerwise.py, 2 e_seq + 2^-17 |ideal|, on tensors with this
    network's statistics (He weights, post-ReLU split-stored inputs of a (1, 64, 80) frame): ideal()
    fed with each defect a kernel can have -- one tap's 16-channel chunk lost at one pixel, every
    w_lo x_hi product lost, every w_hi x_lo product lost, the patch read one column off -- must miss
    the ideal by more than 4x that tolerance, at the mutated pixel for the first and somewhere for
    the others.  Also pins the yardstick itself: a correct f32 accumulation stays inside it."""
    src = R.point_spec(point)[0]
    inp = walked[src]
    _, _, h, w = inp.shape
    pix = R.all_pixels(1, h, w)
    base = R.ideal(point, "bf16x3", inp, rand_weights, pix)
    ks = rand_weights[R.point_spec(point)[1][0][0][0][0]][0].shape[2]
    sample = R.yardstick_pixels(base, ks, np.random.default_rng(point))
    seq = R.seq_f32(point, "bf16x3", inp, rand_weights, pix[sample])
    e_seq = float(np.abs(seq - base[sample]).max())
    tol = R.tolerance(base, e_seq, "bf16x3")
    assert 0.0 < e_seq < 1e-4, e_seq
    assert np.all(np.abs(seq - base[sample]) <= tol[sample])
    pi = (h // 2) * w + w // 2
    found = {}
    for what, mut in (("chunk", {"chunk": (pi, (ks * ks) // 2, 1)}), ("w_lo*x_hi", {"drop": "w_lo*x_hi"}),
                      ("w_hi*x_lo", {"drop": "w_hi*x_lo"}), ("shift", {"shift": 1})):
        got = R.ideal(point, "bf16x3", inp, rand_weights, pix, mutate=mut)
        ratio = np.abs(got - base) / tol
        if what == "chunk":
            assert np.array_equal(np.delete(got, pi, axis=0), np.delete(base, pi, axis=0))
            ratio = ratio[pi]
        found[what] = float(ratio.max())
    print("point %d: e_seq %.2e, defect / tolerance %s" % (point, e_seq, {k: round(v, 1) for k, v in found.items()}))
    assert all(v > 4.0 for v in found.values()), found


@pytest.mark.parametrize("precision,point", [("fp32", 2), ("fp32", 16), ("bf16x3", 3), ("bf16x3", 15)])
def test_another_correct_accumulation_is_inside_the_tolerance(rand_weights, precision, point):
    """The yardstick must not fail a correct kernel: the same f32 sum taken in another order (channels
    backwards) and stored (f32, or the hi/lo pair), at every pixel of a (1, 64, 80) frame's layer, is
    inside 2 e_seq + r |ideal| with e_seq from layer_ref.yardstick_pixels.  (With e_seq from 8 random
    pixels it is not: the largest errors sit at the largest outputs of a few channels, and this
    reordering then needed 2.1 e_seq at conv2_1 and Mconv1 in fp32.)"""
    x = np.random.default_rng(0).uniform(-0.5, 0.5, (1, 3, 64, 80)).astype(np.float32)
    acts = R.walk(rand_weights, x, precision, point)
    inp = acts[R.point_spec(point)[0]]
    _, _, h, w = acts[point].shape
    pix = R.all_pixels(1, h, w)
    want = R.ideal(point, precision, inp, rand_weights, pix)
    got = R.seq_f32(point, precision, inp, rand_weights, pix, reverse=True).astype(np.float32)
    got = (R.recon(got) if precision == "bf16x3" else got).astype(np.float64)
    ks = rand_weights[R.point_spec(point)[1][-1][0][0][0]][0].shape[2]
    sample = R.yardstick_pixels(want, ks, np.random.default_rng(point))
    e_seq = float(np.abs(R.seq_f32(point, precision, inp, rand_weights, pix[sample]) - want[sample]).max())
    err = np.abs(got - want)
    tol = R.tolerance(want, e_seq, precision)
    print("%s point %d: e_seq %.2e, reordered max|err| %.2e, worst err/tol %.2f" % (
        precision, point, e_seq, err.max(), (err / tol).max()))
    assert np.all(err <= tol)


# ---- the CPM nets (net="facenet" / "handnet": the points of op_cpm_forward_probe) ----
CPM_NETS = ("facenet", "handnet")
_cpm_cache = {}


def _cpm_weights(net):
    if ("w", net) not in _cpm_cache:
        from conftest import pkg_module
        _cpm_cache["w", net] = pkg_module("weights").random_weights(seed=4, arch=net)
    return _cpm_cache["w", net]


def _cpm_walked(net):
    """The bf16x3 walk of a (1, 40, 56) frame (5 x 7 maps) up to Mconv1 of stage 2, computed once."""
    if ("walk", net) not in _cpm_cache:
        x = np.random.default_rng(0).uniform(-0.5, 0.5, (1, 3, 40, 56)).astype(np.float32)
        _cpm_cache["walk", net] = R.walk(_cpm_weights(net), x, "bf16x3", 16, net=net)
    return _cpm_cache["walk", net]


@pytest.mark.parametrize("net", CPM_NETS)
def test_cpm_walk_composes_to_the_oracle_forward(net):
    """walk(..., net=) over all 45 points against oracle.cpm.cpm_forward(all_stages=True) on a
    (1, 3, 16, 24) input: the wiring table of layer_ref (which layer reads which point, the pools, the
    (heat, feature) concat out of the padded map point) is the network's.  Two comparisons:
    * fp32 walk (float64 layers, float32 between the points) against the oracle run in float64.  Each
      of the 52 layers adds one float32 rounding (2^-24 relative) to a tensor of He-initialised, ReLU'd
      activations whose perturbations neither grow nor shrink on average, so the maps differ by about
      sqrt(52) 2^-24 = 4e-7 relative r.m.s.; 1e-5 max(1, |map|) leaves the tail of a few thousand
      outputs a factor 5.  A wrong channel, tap or layer is an O(1) relative error.
    * bf16x3 walk against the float32 oracle within the project's forward bound 1e-3
      (tests/test_gpu_cpm.py FWD_TOL, __graft_entry__.smoke)."""
    from oracle import cpm as OC
    W = _cpm_weights(net)
    C = R.CPM_MAPS[net]
    x = np.random.default_rng(1).uniform(-0.5, 0.5, (1, 3, 16, 24)).astype(np.float32)
    W64 = {k: (w.astype(np.float64), b.astype(np.float64)) for k, (w, b) in W.items()}
    ref64 = OC.cpm_forward(W64, x.astype(np.float64), all_stages=True)
    ref32 = OC.cpm_forward(W, x, all_stages=True)
    assert len(ref64) == len(R.MAP_POINTS) and ref64[0].dtype == np.float64
    for precision, ref, bound in (("fp32", ref64, 1e-5), ("bf16x3", ref32, 1e-3)):
        acts = R.walk(W, x, precision, R.N_POINTS - 1, net=net)
        assert sorted(acts) == list(range(R.N_POINTS))
        worst = 0.0
        for s, point in enumerate(R.MAP_POINTS):
            got = acts[point]
            assert got.shape == (1, R.cpm_heat_channels(net) + 128, 2, 3)
            assert not got[:, C:R.cpm_heat_channels(net)].any()
            assert np.array_equal(got[:, R.cpm_heat_channels(net):], acts[R.CPM_FEATURE_POINT])
            err = np.abs(got[:, :C].astype(np.float64) - ref[s])
            worst = max(worst, float((err / np.maximum(1.0, np.abs(ref[s]))).max()))
        print("%s %s walk vs oracle: worst |err| / max(1, |map|) %.3e (bound %.0e)" % (net, precision, worst, bound))
        assert worst <= bound


def _cpm_mconv1(net):
    """Mconv1 of stage 2 (point 16) on the walked map point: ideal at every pixel, e_seq, tolerance."""
    W = _cpm_weights(net)
    inp = _cpm_walked(net)[15]
    _, _, h, w = inp.shape
    pix = R.all_pixels(1, h, w)
    base = R.ideal(16, "bf16x3", inp, W, pix, net=net)
    sample = R.yardstick_pixels(base, 7, np.random.default_rng(16))
    seq = R.seq_f32(16, "bf16x3", inp, W, pix[sample], net=net)
    e_seq = float(np.abs(seq - base[sample]).max())
    tol = R.tolerance(base, e_seq, "bf16x3")
    assert 0.0 < e_seq < 1e-4, e_seq
    assert np.all(np.abs(seq - base[sample]) <= tol[sample])
    return W, inp, pix, base, e_seq, tol


def _with_mconv1(W, Wl):
    out = dict(W)
    out["Mconv1_stage2"] = (np.ascontiguousarray(Wl, np.float32), W["Mconv1_stage2"][1])
    return out


def test_cpm_physical_channel_order():
    """seq_f32 walks Mconv1's input as the kernels do: feature chunks 0..7, then the heat chunks;
    facenet's 13 chunks end in one that is 9/16 padding, handnet has 10."""
    for net, c16, pad in (("facenet", 13, 9), ("handnet", 10, 10)):
        C = R.CPM_MAPS[net]
        src = R._physical_channels(net, "Mconv1_stage2", C + 128)
        assert len(src) == 16 * c16 and np.array_equal(src[:128], C + np.arange(128))
        assert np.array_equal(src[128:128 + C], np.arange(C)) and (src[128 + C:] == -1).all() and (src == -1).sum() == pad
        assert R._physical_channels(net, "Mconv2_stage2", 128) is None
        sel = R.point_spec(16, net)[1][0][0][0][1]
        assert np.array_equal(sel, np.concatenate([np.arange(C), R.cpm_heat_channels(net) + np.arange(128)]))


def test_cpm_tolerance_does_not_hide_a_defect_facenet():
    """2 e_seq + 2^-17 |ideal| at FaceNet's Mconv1 (13 chunks, the last 9/16 padding) and at the map
    point before it, on tensors with the network's statistics.  Each defect must miss the tolerance at
    the outputs it affects (ratio = |defect - ideal| / tolerance > 1; the ratios are printed):
    1. one (tap, chunk) lost at one pixel in the 13th chunk: at that pixel,
    2. the w_lo x_hi products of the 13th chunk lost (its weights kept as bf16 only): somewhere,
    3. Mconv1's weights applied in logical (heat, feature) order to the physical (feature, heat)
       tensor: somewhere,
    4. heat channel C - 1 read from channel C of the padded slice (zero): somewhere."""
    net, C = "facenet", 71
    W, inp, pix, base, e_seq, tol = _cpm_mconv1(net)
    _, _, h, w = inp.shape
    Wl = W["Mconv1_stage2"][0]
    found = {}
    pi = (h // 2) * w + w // 2
    got = R.ideal(16, "bf16x3", inp, W, pix, mutate={"chunk": (pi, 24, 12)}, net=net)
    assert np.array_equal(np.delete(got, pi, axis=0), np.delete(base, pi, axis=0))
    # the lost terms are the 7 heat channels 64..70 of the centre tap
    assert inp[0, 64:71, h // 2, w // 2].any()
    found["chunk"] = float((np.abs(got - base) / tol)[pi].max())
    W2 = Wl.copy()
    W2[:, 64:71] = R.bf16_rne(Wl[:, 64:71])  # split() of a bf16 value is (hi, 0): no w_lo x_hi term
    found["w_lo*x_hi"] = float((np.abs(R.ideal(16, "bf16x3", inp, _with_mconv1(W, W2), pix, net=net) - base) / tol).max())
    src = R._physical_channels(net, "Mconv1_stage2", C + 128)
    W3 = np.empty_like(Wl)
    phys = np.arange(C + 128)
    W3[:, src[phys]] = Wl[:, phys]  # physical channel p (logical src[p]) meets the weights of logical channel p
    found["logical order"] = float((np.abs(R.ideal(16, "bf16x3", inp, _with_mconv1(W, W3), pix, net=net) - base) / tol).max())
    inp4 = inp.copy()
    inp4[:, C - 1] = inp[:, C]
    assert not inp[:, C].any() and inp[:, C - 1].any()
    found["slice off by one"] = float((np.abs(R.ideal(16, "bf16x3", inp4, W, pix, net=net) - base) / tol).max())
    print("facenet Mconv1_stage2: e_seq %.2e, defect / tolerance %s" % (e_seq, {k: round(v, 1) for k, v in found.items()}))
    assert all(v > 1.0 for v in found.values()), found


def test_cpm_tolerance_does_not_hide_a_dropped_split_k_half_handnet():
    """5. HandNet's Mconv1 has 10 chunks; a 2-way K split sums chunks 0..4 and 5..9 apart.  Either half
    lost (its weights zero: physical channels 0..79 = feature 0..79, or 80..159 = feature 80..127 and
    the heat) misses the tolerance."""
    net, C = "handnet", 22
    W, inp, pix, base, e_seq, tol = _cpm_mconv1(net)
    Wl = W["Mconv1_stage2"][0]
    src = R._physical_channels(net, "Mconv1_stage2", C + 128)
    found = {}
    for half in (0, 1):
        lost = src[80 * half:80 * half + 80]
        W5 = Wl.copy()
        W5[:, lost[lost >= 0]] = 0
        got = R.ideal(16, "bf16x3", inp, _with_mconv1(W, W5), pix, net=net)
        found["half %d" % half] = float((np.abs(got - base) / tol).max())
    print("handnet Mconv1_stage2: e_seq %.2e, defect / tolerance %s" % (e_seq, {k: round(v, 1) for k, v in found.items()}))
    assert all(v > 1.0 for v in found.values()), found


def test_cpm_stored_pairs_decide_at_a_bf16_tie():
    """inputs_hi: with the hi halves split() gives, the ideal and the yardstick are those without,
    bit for bit.  A stored value exactly halfway between two bf16 values can be either (lower, +half a
    step) or (upper, -half); given the other pair, the ideal moves by w_lo times the step at the
    outputs that read it (HandNet Mconv2 of stage 2, a 7x7 layer) and nowhere else."""
    net = "handnet"
    W = _cpm_weights(net)
    inp = _cpm_walked(net)[16].copy()
    _, _, h, w = inp.shape
    pix = R.all_pixels(1, h, w)
    inp[0, 5, 2, 3] = np.float32(2.1015625)  # 2.09375 + 2^-7 = 2.109375 - 2^-7
    hi = R.bf16_rne(inp)
    assert hi[0, 5, 2, 3] == np.float32(2.09375)
    base = R.ideal(17, "bf16x3", inp, W, pix, net=net)
    assert np.array_equal(R.ideal(17, "bf16x3", inp, W, pix, net=net, inputs_hi=hi), base)
    some = pix[::5]
    assert np.array_equal(R.seq_f32(17, "bf16x3", inp, W, some, net=net, inputs_hi=hi), R.seq_f32(17, "bf16x3", inp, W, some, net=net))
    hi[0, 5, 2, 3] = np.float32(2.109375)
    got = R.ideal(17, "bf16x3", inp, W, pix, net=net, inputs_hi=hi)
    w_lo = R.split(W["Mconv2_stage2"][0])[1].astype(np.float64)  # (Co, Ci, 7, 7)
    want = base.copy()
    for i, (_, y, x) in enumerate(pix):
        dy, dx = 2 - y + 3, 3 - x + 3  # the tap of output (y, x) that reads input pixel (2, 3)
        if 0 <= dy < 7 and 0 <= dx < 7:
            want[i] += w_lo[:, 5, dy, dx] * 2.0 ** -6
    live = (base > 1e-3) & (want > 1e-3)  # (away from the ReLU)
    assert live.sum() > 1000 and np.abs(got - want)[live].max() <= 1e-12
    print("other pair at one input: ideal moves by up to %.2e" % np.abs(got - base).max())
    assert np.abs(got - base).max() > 1e-6
