"""Every launch of the training backward held to its own reference (op_train_read_buffer,
oracle/train_ref.py).

One step per configuration (tests/train_layerwise.py CONFIGS: the smallest shapes that reach each
branch of tr_backward) is run once and its 89 activation and 89 gradient buffers are read back.  After
a step the gradient buffer of a conv output holds the masked dY_pre and every activation is resident,
so each launch is recomputed in float64 from the device's own operands and the weights the step was
given:

* exact: the stage-6 map gradient is the loss-gradient formula; a pool input's gradient is
  where(first maximum and Y > 0, dP, 0); every gradient is 0 where the producer's Y <= 0; physical
  channels nothing writes stay 0; buffers below the lowest enabled layer stay 0;
* input gradients, all channels of the checked pixels:
  |g - ideal| <= 2 sum_consumers e_seq + k 2^-23 sum |terms| (train_layerwise.check_input_gradient);
* weight and bias gradients, every entry: |dW - ideal| <= 2 e_seq + 2^-23 |ideal|
  (train_layerwise.check_weight_gradient).

tests/test_train_ref.py pins the reference's wiring to float64 autograd and shows what the
tolerances catch.  Every check prints max |err|, e_seq, their ratio and the factor on e_seq it needed
(DESIGN.md §2b has the table)."""
import ctypes

import numpy as np
import pytest

import train_layerwise as TL
from conftest import pkg_module
from oracle import train_ref as TR

pytestmark = pytest.mark.gpu

G = TR.graph()
NODES = ["%s:%s" % k for k in G.order]
LAYERS = [c.name for c in G.convs]
_runs = {}
_failed = []


def _setup(ctx, cfg, W0):
    """Weights, the reference hook's multipliers and the frozen layers, as tests/test_gpu_train.py."""
    ctx.set_weights(W0)
    ctx.set_hyper(1e-4)
    names = [t[0] for t in ctx.table]
    for nm, sc in TL.hook_multipliers().items():
        if sc != 1.0:
            ctx.set_grad_scale(names.index(nm), sc)
    frozen = pkg_module("train").VGG_FROZEN if cfg.get("frozen") else []
    for nm in frozen:
        ctx.enable(names.index(nm), False)
    return frozen


def _run(name):
    """The configuration's step: its tensors, gradients and inputs, read once."""
    if _failed:  # a step that failed is not tried again, nor is any other started behind it
        pytest.fail("the step of %s failed: %s" % _failed[0])
    if name not in _runs:
        lib = pkg_module("_lib")
        cfg = TL.CONFIGS[name]
        n, h, w = cfg["shape"]
        W0 = TL.config_weights(cfg, pkg_module("weights").random_weights(seed=7))
        x, pt, ht, ig = TL.data(n, h, w, 3)
        ctx = lib.TrainContext(n, h, w, 0)
        try:
            frozen = _setup(ctx, cfg, W0)
            ctx.step(x, pt, ht, ig)
            grads = ctx.get(grads=True)
            T = TR.Tensors()
            for i in range(len(G.bufs)):
                T._a[i] = ctx.read(i)
                T._g[i] = ctx.read(i, grad=True)
        except Exception as e:
            _failed.append((name, e))
            raise
        finally:
            ctx.close()
        lowest = min(c.layer for c in G.convs if c.name not in frozen)
        _runs[name] = dict(T=T, grads=grads, W0=W0, targets=dict(pafs=pt, heat=ht, ign=ig), n=n, frozen=frozen,
                           lowest=lowest)
    return _runs[name]


@pytest.mark.parametrize("node", NODES)
@pytest.mark.parametrize("config", list(TL.CONFIGS))
def test_node_gradient_vs_single_launch_reference(config, node):
    run = _run(config)
    T = run["T"]
    kind, idx = node.split(":")
    nd = G.nodes[(kind, int(idx))]
    got = T.grad(nd.buf)[:, nd.c0:nd.c1]
    if nd.relu:  # exact: nothing where the producer's ReLU clamped
        assert not got[~(T.act(nd.buf)[:, nd.c0:nd.c1] > 0)].any(), nd.name
    if nd.kind == "conv" and nd.layer < run["lowest"]:
        assert not got.any(), nd.name  # the backward stops at the lowest enabled layer
        return
    pi = TR.pooled_by(G, nd)
    if pi is not None:  # exact: the pooled gradient at the first maximum of each window
        y = T.act(nd.buf)
        want = np.where(y > 0, TR.pool_route(y, T.grad(G.pools[pi][1])), 0)
        assert np.array_equal(got, want), nd.name
        if TL.CONFIGS[config].get("ties") and nd.name == "conv3_4":
            assert not got[:, :, 1::2].any() and not got[:, :, :, 1::2].any() and got.any()
        return
    r = TL.check_input_gradient(G, nd, T, run["W0"], run["targets"], run["n"], run["lowest"])
    print(TL.line("dX", config, nd.name, r) + " terms %d at %s" % (r["terms"], r["at"]))
    assert r["masked_nonzero"] == 0 and r["bad"] == 0, (nd.name, r["worst"], r["need"], r["at"])


@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("config", list(TL.CONFIGS))
def test_weight_gradient_vs_single_launch_reference(config, layer):
    run = _run(config)
    cv = G.convs[LAYERS.index(layer)]
    gW, gb = run["grads"][layer]
    if layer in run["frozen"]:
        assert not gW.any() and not gb.any()  # a disabled layer reports zeros
        return
    r = TL.check_weight_gradient(cv, run["T"], gW, gb)
    print(TL.line("dW", config, layer, r["W"]))
    print(TL.line("db", config, layer, r["b"]))
    assert r["W"]["bad"] == 0 and r["b"]["bad"] == 0, (layer, r["W"]["worst"], r["b"]["worst"])


@pytest.mark.parametrize("config", list(TL.CONFIGS))
def test_exact_properties_of_the_step(config):
    run = _run(config)
    T, tg = run["T"], run["targets"]
    # the stage-6 map gradient is the loss gradient, bit for bit
    y, g = T.act(G.out6), T.grad(G.out6)
    assert np.array_equal(g[:, 0:38], TR.loss_gradient(y[:, 0:38], tg["pafs"], tg["ign"]))
    assert np.array_equal(g[:, 40:59], TR.loss_gradient(y[:, 40:59], tg["heat"], tg["ign"]))
    assert g[:, 0:38].any() and g[:, 40:59].any()
    # physical channels nothing writes
    for arr in (y, g):
        assert not arr[:, 38:40].any() and not arr[:, 59:64].any()
    for b in G.cat:
        for arr in (T.act(b), T.grad(b)):
            assert not arr[:, 147:152].any() and not arr[:, 190:192].any()
    assert not T.act(0)[:, 3:].any()
    # the feature copies
    for s in range(1, 5):
        assert np.array_equal(T.act(G.cat[s])[:, :128], T.act(G.cat[0])[:, :128])
    # buffers wholly below the lowest enabled layer
    if run["frozen"]:
        top = G.convs[run["lowest"]].inb
        assert run["lowest"] == 10 and G.bufs[top][0] == "conv4_2"
        for i in range(top + 1):
            assert not T.grad(i).any(), G.bufs[i]
        assert T.grad(top + 1).any()
    else:
        assert not T.grad(0).any()  # conv1_1 has no input gradient
        # (conv3_4's zero weights of the tie case pass nothing on below it)
        assert T.grad(G.convs[7].out if TL.CONFIGS[config].get("ties") else 1).any()


def test_read_back_does_not_disturb_the_state():
    lib = pkg_module("_lib")
    cfg = TL.CONFIGS["1x40x40"]
    n, h, w = cfg["shape"]
    W0 = pkg_module("weights").random_weights(seed=7)
    a, b = TL.data(n, h, w, 3), TL.data(n, h, w, 4)
    out = []
    for reads in (False, True):
        ctx = lib.TrainContext(n, h, w, 0)
        try:
            _setup(ctx, cfg, W0)
            l1 = ctx.step(*a)
            if reads:
                for i, grad in ((0, False), (15, True), (22, True), (88, True), (40, False)):
                    ctx.read(i, grad=grad)
            l2 = ctx.step(*b)
            out.append((l1, l2, ctx.get(), ctx.get(grads=True), ctx.get_state()))
        finally:
            ctx.close()
    (p1, p2, pw, pg, ps), (r1, r2, rw, rg, rs) = out
    assert np.array_equal(p1, r1) and np.array_equal(p2, r2)
    for nm in pw:
        for k in (0, 1):
            assert np.array_equal(pw[nm][k], rw[nm][k]) and np.array_equal(pg[nm][k], rg[nm][k]), nm
        for key in ("mW", "vW", "mb", "vb"):
            assert np.array_equal(ps[nm][key], rs[nm][key]), (nm, key)
        assert ps[nm]["t"] == rs[nm]["t"] == 2


def test_read_buffer_arguments():
    lib = pkg_module("_lib")
    L = lib.lib()
    table = lib.train_buffer_table()
    assert table == G.bufs
    n, h, w = 1, 16, 24
    ctx = lib.TrainContext(n, h, w, 0)
    try:
        ctx.set_weights(pkg_module("weights").random_weights(seed=7))
        out = np.empty((n, 64, 2, 3), np.float32)
        assert L.op_train_read_buffer(ctx.h_, 88, 0, lib.ptr(out), out.size) == lib.OP_ERR_STATE
        x, pt, ht, ig = TL.data(n, h, w, 3)
        ctx.step(x, pt, ht, ig)
        assert L.op_train_read_buffer(ctx.h_, 88, 0, lib.ptr(out), out.size) == lib.OP_OK
        for bad in ((-1, out.size), (89, out.size), (88, out.size - 1), (88, out.size + 1), (87, out.size)):
            assert L.op_train_read_buffer(ctx.h_, bad[0], 1, lib.ptr(out), bad[1]) == lib.OP_ERR_INVALID, bad
            assert lib.last_error()
        assert L.op_train_read_buffer(ctx.h_, 88, 1, None, out.size) == lib.OP_ERR_INVALID
        # the network input comes back as given
        assert np.array_equal(ctx.read(0)[:, :3], x)
    finally:
        ctx.close()
    name, ch, div = ctypes.c_char_p(), ctypes.c_int32(), ctypes.c_int32()
    for i in (-1, 89):
        assert L.op_train_buffer_info(i, ctypes.byref(name), ctypes.byref(ch), ctypes.byref(div)) == lib.OP_ERR_INVALID
