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
