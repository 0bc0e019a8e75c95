"""oracle/train_ref.py, the single-launch reference of tests/test_gpu_train_layerwise.py, checked on
the CPU: its wiring against float64 autograd of the whole iteration, its yardsticks against a correct
f32 sum in another order, and its tolerances against the defects they have to catch."""
import numpy as np
import pytest

import train_layerwise as TL
from conftest import pkg_module
from oracle import layer_ref as R
from oracle import train_ref as TR

torch = pytest.importorskip("torch")

SHAPES = [(1, 24, 40), (2, 16, 16), (1, 32, 40)]
_steps = {}


def _step(shape):
    """The float64 step at `shape` (weights seed 7, data seed 3): (G, W, targets, T float64, grads)."""
    if shape not in _steps:
        n, h, w = shape
        G = TR.graph()
        W = pkg_module("weights").random_weights(seed=7)
        x, pt, ht, ig = TL.data(n, h, w, 3)
        targets = dict(pafs=pt, heat=ht, ign=ig)
        T = TR.forward(G, W, x)
        grads = TR.backward(G, W, T, targets)
        _steps[shape] = (G, W, (x, pt, ht, ig), targets, T, grads)
    return _steps[shape]


def _rounded(T):
    """The float64 step's tensors rounded to f32: tensors with the statistics of the device's."""
    T32 = TR.Tensors()
    T32._a = {i: a.astype(np.float32) for i, a in T._a.items()}
    T32._g = {i: g.astype(np.float32) for i, g in T._g.items()}
    return T32


@pytest.fixture(scope="module")
def step32():
    G, W, _, targets, T, _ = _step((1, 32, 40))
    return G, W, targets, _rounded(T)


def test_graph_is_the_library_buffer_table(lib):
    G = TR.graph()
    assert G.bufs == lib.train_buffer_table()
    assert len(G.bufs) == lib.N_TRAIN_BUFFERS and len(G.convs) == 92
    assert sorted(G.order) == sorted(G.nodes) and len(G.order) == 92 + 3 + 4


@pytest.mark.parametrize("shape", SHAPES)
def test_chained_ideals_are_float64_autograd(shape):
    """The per-node ideals chained from the loss down, each fed its own float64 output, give the 92
    (dW, db) of torch's float64 autograd to 1e-9 relative: pins graph(), the channel maps, the flipped
    taps, the pool routing, the loss term and the feature adds without a GPU."""
    G, W, (x, pt, ht, ig), _, T, grads = _step(shape)
    _, ref = TL.torch_step(W, x, pt, ht, ig)
    assert sorted(grads) == sorted(ref)
    for name in ref:
        for got, want in zip(grads[name], ref[name]):
            assert got.shape == want.shape, name
            assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), name


def test_wgrad_split_restates_the_launch():
    # (total pixels) -> (splits, pps): the cases tests/train_layerwise.py CONFIGS names
    assert TR.wgrad_split(6144) == (12, 512) and TR.wgrad_split(96) == (1, 96)
    assert TR.wgrad_split(1600) == (3, 544) and TR.wgrad_split(100) == (1, 112) and TR.wgrad_split(25) == (1, 32)
    assert TR.wgrad_split(32832) == (64, 528) and 62 * 528 + 96 == 32832  # the 63rd split 96 px, the 64th empty
    assert TR.wgrad_split(45) == (1, 48) and TR.wgrad_split(180) == (1, 192)


# ---- yardsticks: another correct f32 order stays inside the tolerance ----
@pytest.mark.parametrize("name", ["conv1_1", "conv4_3_CPM", "conv4_4_CPM", "conv5_4_CPM_L1", "conv5_5_CPM_L2",
                                  "Mconv2_stage3_L1", "pool2"])
def test_input_gradient_in_another_order_is_inside_the_tolerance(step32, name):
    """The node's addends accumulated in f32 with the channels walked backwards, rounded and added one
    after the other in f32, masked: a correct kernel in another order."""
    G, W, targets, T = step32
    node = [nd for nd in G.nodes.values() if nd.name == name][0]
    base = TL.check_input_gradient(G, node, T, W, targets, 1)
    pix = base["pix"]
    acc = np.zeros(base["ideal"].shape, np.float32)
    for cv, v in TR.node_terms(G, node, T, W, pix, targets):
        v = TR.input_term_seq(cv, node, T, W, pix, reverse=True) if cv is not None else v
        acc = acc + v.astype(np.float32)
    got = np.where(base["mask"], acc, 0).astype(np.float64)
    r = TL.check_input_gradient(G, node, T, W, targets, 1, got=got)
    print(TL.line("dX reordered", "1x32x40", name, r))
    assert r["e_seq"] > 0 and r["bad"] == 0 and r["masked_nonzero"] == 0, r["worst"]


@pytest.mark.parametrize("name", ["conv1_2", "conv2_2", "conv4_2", "Mconv1_stage2_L1", "Mconv7_stage6_L1"])
def test_weight_gradient_in_another_order_is_inside_the_tolerance(step32, name):
    """dW (8192 random entries and the yardstick's own) and db summed over the pixels backwards."""
    G, W, targets, T = step32
    cv = [c for c in G.convs if c.name == name][0]
    dW, db = TR.weight_gradient(cv, T)
    rng = np.random.default_rng(5)
    size = dW.size
    pick = np.unravel_index(rng.choice(size, min(8192, size), replace=False), (cv.co, cv.ci, cv.k * cv.k))
    got = dW.reshape(cv.co, cv.ci, -1).copy()  # entries not re-summed stay ideal
    got[pick] = TR.weight_gradient_seq(cv, T, pick, reverse=True)
    r = TL.check_weight_gradient(cv, T, got.reshape(dW.shape), TR.bias_gradient_seq(cv, T, reverse=True))
    print(TL.line("dW reordered", "1x32x40", name, r["W"]))
    print(TL.line("db reordered", "1x32x40", name, r["b"]))
    assert r["W"]["bad"] == 0 and r["b"]["bad"] == 0, (r["W"]["worst"], r["b"]["worst"])


# ---- sensitivity: every defect misses its check by 4x or more ----
def _node(G, name):
    return [nd for nd in G.nodes.values() if nd.name == name][0]


def _conv(G, name):
    return [c for c in G.convs if c.name == name][0]


@pytest.mark.parametrize("name", ["conv1_2", "conv4_2", "conv5_5_CPM_L1", "Mconv3_stage3_L1"])
def test_a_dropped_pixel_of_one_tap_misses_the_weight_gradient_tolerance(step32, name):
    """The last pixel of the launch (at /8: 20 px, the 4th of a partial 16-pixel step) left out of the
    centre tap's sum."""
    G, W, targets, T = step32
    cv = _conv(G, name)
    g, shifted = TR._wgrad_operands(cv, T)
    tap = (cv.k * cv.k) // 2
    dW, db = TR.weight_gradient(cv, T)
    bad = dW.reshape(cv.co, cv.ci, -1).copy()
    bad[:, :, tap] -= np.outer(g[-1].astype(np.float64), shifted(tap)[-1].astype(np.float64))
    r = TL.check_weight_gradient(cv, T, bad.reshape(dW.shape), db)
    print("SENSITIVITY dropped pixel %s: defect / tolerance %.1f" % (name, r["W"]["worst"]))
    assert r["W"]["worst"] > 4.0


@pytest.mark.parametrize("name", ["conv1_1", "conv1_2"])
def test_a_dropped_bias_partial_misses_the_tolerance(step32, name):
    G, W, targets, T = step32
    cv = _conv(G, name)
    g, _ = TR._wgrad_operands(cv, T)
    splits, pps = TR.wgrad_split(g.shape[0])
    assert splits == 2
    dW, db = TR.weight_gradient(cv, T)
    r = TL.check_weight_gradient(cv, T, dW, db - g[pps:].astype(np.float64).sum(axis=0))
    print("SENSITIVITY dropped bias partial %s: defect / tolerance %.1f" % (name, r["b"]["worst"]))
    assert r["b"]["worst"] > 4.0


@pytest.mark.parametrize("what,name", [("noflip", "conv4_3_CPM"), ("noflip", "Mconv2_stage2_L2"),
                                       ("drop_group", "conv5_4_CPM_L1"), ("drop_group", "Mconv6_stage4_L1"),
                                       ("relu_ge", "conv5_2_CPM_L1"), ("relu_ge", "conv3_1"),
                                       ("no_ignore", "conv5_5_CPM_L1"), ("no_ignore", "Mconv7_stage3_L2")])
def test_an_input_gradient_defect_misses_the_tolerance(step32, what, name):
    """Taps not flipped; the last 8-channel group (32..37) of the 38-channel PAF dY lost at one pixel of
    its 1x1 input-gradient conv; the ReLU mask taken as Y >= 0; the ignore mask not applied to dY."""
    G, W, targets, T = step32
    node = _node(G, name)
    mutate = {what: True}
    if what == "drop_group":
        paf = [c for c in TR.consumers(G, node) if c.co == 38]
        assert len(paf) == 1 and paf[0].k == 1
        mutate = {"drop_group": (paf[0].layer, 7)}
    r = TL.check_input_gradient(G, node, T, W, targets, 1, mutate=mutate)
    print("SENSITIVITY %s %s: defect / tolerance %.1f (masked elements made nonzero: %d)" % (
        what, name, r["worst"], r["masked_nonzero"]))
    assert r["worst"] > 4.0
    if what == "relu_ge":
        assert r["masked_nonzero"] > 0  # the exact check sees it too
    if what == "drop_group":
        assert r["at"][0] == int(r["pix"][7, 0]) and r["at"][2:] == tuple(int(v) for v in r["pix"][7, 1:])


def test_the_last_maximum_of_a_tied_window_is_not_the_first():
    """The pool check is exact, so any misrouting fails it; here: routing to the last maximum differs
    from pool_route wherever a window ties, and only there."""
    rng = np.random.default_rng(0)
    X = rng.uniform(0, 1, (2, 3, 6, 8)).astype(np.float32)
    X[0] = 0.5  # every window of frame 0 ties
    dP = rng.uniform(-1, 1, (2, 3, 3, 4)).astype(np.float32)
    first, last = TR.pool_route(X, dP), TR.pool_route(X, dP, last=True)
    assert np.array_equal(first[1], last[1]) and not np.array_equal(first[0], last[0])
    assert np.array_equal(first[0, :, 0::2, 0::2], dP[0]) and not first[0, :, 1::2, 1::2].any()
    assert np.array_equal(last[0, :, 1::2, 1::2], dP[0])
    assert float(first.sum(dtype=np.float64)) == float(dP.sum(dtype=np.float64))


def test_loss_gradient_formula():
    rng = np.random.default_rng(1)
    y = rng.uniform(-1, 1, (2, 38, 3, 5)).astype(np.float32)
    t = rng.uniform(-1, 1, y.shape).astype(np.float32)
    ign = rng.random((2, 3, 5)) < 0.3
    g = TR.loss_gradient(y, t, ign)
    assert g.dtype == np.float32 and not g[np.broadcast_to(ign[:, None], y.shape)].any()
    want = 2.0 * (y.astype(np.float64) - t) / y.size
    keep = ~np.broadcast_to(ign[:, None], y.shape)
    assert np.abs(g[keep] - want[keep]).max() <= 2.0 ** -22 * np.abs(want).max()
