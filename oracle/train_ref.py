"""ORACLE — TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

Single-launch reference of the training backward (csrc/train.hip tr_backward), evaluated in float64
from the tensors the device itself holds after a step (``op_train_read_buffer``): after a step the
gradient buffer of a conv output holds the masked ``dY_pre`` (tr_relu_bwd works in place) and every
activation is still resident, so each launch can be recomputed from its own operands.  Our own NumPy
code; nothing here restates the reference project beyond the layer wiring of
models/CocoPoseNet.py:132-262 and compute_loss (train_coco_pose_estimation.py:42-77).

The wiring (``graph``) comes from the layer table (oracle/forward.py LAYERS): the step's buffers in
the order ``op_train_buffer_info`` reports them, one conv per layer with its input / output buffer
and channel slices, the pools, and the physical channel map of the 192-channel stage inputs
(feature 0..127, heat 128..146, paf 152..189).  The backward is organised by *nodes*: a node is a
channel slice of a gradient buffer that one thing produces (a conv output, a pool output, or the
feature copy in the stage 3-6 inputs), and its gradient is

    mask( sum over consumer convs of conv(dY_pre, W') + loss term + feature-copy gradients )

with W' the flipped taps, the loss term ``f32(f32(y - t) * f32(2 / numel))`` (zero where ignored) on
the map slices of stages 1-6, the feature gradients of the stage 3-6 inputs added at conv4_4_CPM's
output (tr_add at layer 11), and the mask ``Y > 0`` of the producing ReLU.  A conv output that a
pool reads gets the pooled gradient at the first maximum of each window in (ky, kx) order.

Weight gradient: ``dW[co][ci][tap] = sum_p dY_pre[p][co] X[p + tap][ci]``, ``db[co] = sum_p
dY_pre[p][co]``.

Yardsticks (the same terms in float32, one at a time, in the kernels' order):

* input gradient: layer_ref._gemm_seq's exact path (16-channel chunk, tap, channel over the
  channels of dY_pre) on the flipped weights: the input-gradient conv is the forward's exact-f32
  kernel (conv.hip) launched on dY_pre;
* weight gradient: one FMA per pixel in raster order within a split of ``pps`` pixels, then the
  splits added in order (tr_wgrad / tr_wreduce; ``splits`` and ``pps`` restated from tr_backward);
  the bias the same with plain adds (tr_wgrad's ``bacc``, tr_breduce).
"""
import collections

import numpy as np

from . import layer_ref as R
from .forward import LAYERS

CAT_STRIDE, CAT_FEAT, CAT_HEAT, CAT_PAF = 192, 0, 128, 152  # csrc/common.hpp kCat*
WG_PX = 16  # tr_wgrad's pixel step (kWgPx)

Conv = collections.namedtuple("Conv", "layer name ci co k inb cin_off cin_phys out cout_off store relu cat")
Node = collections.namedtuple("Node", "kind layer buf c0 c1 relu name")
Graph = collections.namedtuple("Graph", "bufs convs pools nodes order cat out6")


def cat_logical():
    """(192,) physical channel of a stage input -> logical input channel of Mconv1 (paf 0..37, heat
    38..56, feature 57..184), -1 where nothing lives (train.hip tr_pack / tr_wreduce)."""
    m = np.full(CAT_STRIDE, -1, np.int64)
    m[CAT_FEAT:CAT_FEAT + 128] = 57 + np.arange(128)
    m[CAT_HEAT:CAT_HEAT + 19] = 38 + np.arange(19)
    m[CAT_PAF:CAT_PAF + 38] = np.arange(38)
    return m


def graph():
    """The step's buffers, convs and gradient nodes from the layer table (train.hip build_graph)."""
    names = [l[0] for l in LAYERS]
    dims = {n: (ci, co, k) for n, ci, co, k in LAYERS}
    bufs, index = [], {}

    def buf(name, ch, div):
        index[name] = len(bufs)
        bufs.append((name, ch, div))
        return index[name]

    buf("input", 8, 1)
    div = 1
    pool_after = {"conv1_2": "pool1", "conv2_2": "pool2", "conv3_4": "pool3"}
    for name in names[:11]:  # conv1_1 .. conv4_3_CPM: one buffer per output
        buf(name, dims[name][1], div)
        if name in pool_after:
            div *= 2
            buf(pool_after[name], dims[name][1], div)
    cat = [buf("stage%d_input" % s, CAT_STRIDE, 8) for s in range(2, 7)]
    for b in (1, 2):
        for i in (1, 2, 3, 4):
            n = "conv5_%d_CPM_L%d" % (i, b)
            buf(n, dims[n][1], 8)
    for s in range(2, 7):
        for b in (1, 2):
            for i in range(1, 7):
                n = "Mconv%d_stage%d_L%d" % (i, s, b)
                buf(n, dims[n][1], 8)
    out6 = buf("stage6_maps", 64, 8)

    convs, pools = [], []

    def conv(name, inb, cin_off, out, cout_off, store, relu, is_cat=False):
        ci, co, k = dims[name]
        convs.append(Conv(names.index(name), name, ci, co, k, inb, cin_off, CAT_STRIDE if is_cat else (ci + 7) // 8 * 8,
                          out, cout_off, store, relu, is_cat))

    prev = 0
    for name in names[:11]:
        conv(name, prev, 0, index[name], 0, dims[name][1], True)
        prev = index[name]
        if name in pool_after:
            pools.append((index[name], index[pool_after[name]]))
            prev = index[pool_after[name]]
    conv("conv4_4_CPM", prev, 0, cat[0], CAT_FEAT, 128, True)
    for b in (1, 2):
        prev, off = cat[0], CAT_FEAT
        for i in (1, 2, 3, 4):
            n = "conv5_%d_CPM_L%d" % (i, b)
            conv(n, prev, off, index[n], 0, dims[n][1], True)
            prev, off = index[n], 0
        conv("conv5_5_CPM_L%d" % b, prev, 0, cat[0], CAT_PAF if b == 1 else CAT_HEAT, 40 if b == 1 else 20, False)
    for s in range(2, 7):
        for b in (1, 2):
            prev = cat[s - 2]
            for i in range(1, 7):
                n = "Mconv%d_stage%d_L%d" % (i, s, b)
                conv(n, prev, 0, index[n], 0, dims[n][1], True, is_cat=(i == 1))
                prev = index[n]
            if s == 6:
                dst, off = out6, (0 if b == 1 else 40)
            else:
                dst, off = cat[s - 1], (CAT_PAF if b == 1 else CAT_HEAT)
            conv("Mconv7_stage%d_L%d" % (s, b), prev, 0, dst, off, 40 if b == 1 else 20, False)
    convs.sort(key=lambda c: c.layer)
    assert [c.layer for c in convs] == list(range(len(LAYERS)))

    nodes = {}
    for c in convs:
        nodes[("conv", c.layer)] = Node("conv", c.layer, c.out, c.cout_off, c.cout_off + c.store, c.relu, c.name)
    for i, (src, dst) in enumerate(pools):
        nodes[("pool", i)] = Node("pool", None, dst, 0, bufs[dst][1], False, bufs[dst][0])
    for s in range(1, 5):
        nodes[("copy", s)] = Node("copy", None, cat[s], CAT_FEAT, CAT_FEAT + 128, False, bufs[cat[s]][0] + ":feature")
    # a reverse topological order: every node after all of its consumers
    pool_src = {src: i for i, (src, dst) in enumerate(pools)}
    order = []
    for c in reversed(convs):
        if c.name == "conv4_4_CPM":
            order += [("copy", s) for s in range(1, 5)]
        if c.out in pool_src:
            order.append(("pool", pool_src[c.out]))
        order.append(("conv", c.layer))
    return Graph(bufs, convs, pools, nodes, order, cat, out6)


def wgrad_split(total):
    """(splits, pps) of tr_backward's weight-gradient launch over `total` output pixels."""
    splits = max(1, min(64, total // 512))
    pps = ((total + splits - 1) // splits + WG_PX - 1) // WG_PX * WG_PX
    return splits, pps


class Tensors(object):
    """act(i) / grad(i): buffer i as (n, physical channels, h, w).  `read(i, grad)` supplies them (the
    device's read-back, cached here) or they are set directly (the CPU chain)."""

    def __init__(self, read=None):
        self._read = read
        self._a, self._g = {}, {}

    def act(self, i):
        if i not in self._a:
            self._a[i] = self._read(i, False)
        return self._a[i]

    def grad(self, i):
        if i not in self._g:
            self._g[i] = self._read(i, True)
        return self._g[i]


def _gather(a, pix, ks):
    """a (n, C, h, w), pix (P, 3) -> (P, taps, C): the ks x ks patch around each pixel, zero outside."""
    r = ks // 2
    ap = np.pad(a, ((0, 0), (0, 0), (r, r), (r, r))) if r else a
    out = np.empty((len(pix), ks * ks, a.shape[1]), a.dtype)
    for t in range(ks * ks):
        out[:, t] = ap[pix[:, 0], :, pix[:, 1] + t // ks, pix[:, 2] + t % ks]
    return out


def _at(a, pix, c0, c1):
    return a[pix[:, 0], c0:c1, pix[:, 1], pix[:, 2]]


def _node_channels(cv, node):
    """(columns of the node, logical input channels of cv) the conv's input gradient lands in."""
    p = np.arange(node.c0, node.c1)
    if cv.cat:
        lg = cat_logical()[p]
    else:
        lg = p - cv.cin_off
        lg = np.where((lg >= 0) & (lg < cv.ci), lg, -1)
    ok = lg >= 0
    return np.nonzero(ok)[0], lg[ok]


def _flipped(W, flip=True):
    """W (Co, Ci, k, k) -> (taps, Co, Ci) of the input-gradient conv: W'[tap][co][ci] = W[co][ci][taps-1-tap]."""
    co, ci = W.shape[:2]
    w = W.reshape(co, ci, -1)
    if flip:
        w = w[:, :, ::-1]
    return np.ascontiguousarray(w.transpose(2, 0, 1))


def consumers(G, node, lowest=0):
    """The convs whose input gradient is added into the node (those the backward runs: layer > lowest)."""
    out = []
    for cv in G.convs:
        if cv.inb != node.buf or cv.layer <= max(lowest, 0):
            continue
        if len(_node_channels(cv, node)[0]):
            out.append(cv)
    return out


def input_term(cv, node, T, weights, pix, mutate=None):
    """conv(dY_pre, W') of consumer cv at pixels pix, in the node's columns -> (P, c1 - c0) float64."""
    mutate = mutate or {}
    dy = T.grad(cv.out)[:, cv.cout_off:cv.cout_off + cv.co]
    xg = _gather(dy, pix, cv.k).astype(np.float64)
    if mutate.get("drop_group") and mutate["drop_group"][0] == cv.layer:  # the last 8-channel group lost at one pixel
        xg[mutate["drop_group"][1], :, (cv.co - 1) // 8 * 8:] = 0.0
    cols, lg = _node_channels(cv, node)
    Wp = _flipped(np.asarray(weights[cv.name][0], np.float64), not mutate.get("noflip"))[:, :, lg]
    out = np.zeros((len(pix), node.c1 - node.c0))
    out[:, cols] = xg.reshape(len(pix), -1) @ Wp.reshape(-1, len(lg))
    return out


def input_term_seq(cv, node, T, weights, pix, reverse=False):
    """The same term accumulated in float32 in the conv kernel's order (layer_ref._gemm_seq)."""
    dy = T.grad(cv.out)[:, cv.cout_off:cv.cout_off + cv.co]
    xg = _gather(np.asarray(dy, np.float32), pix, cv.k)
    cols, lg = _node_channels(cv, node)
    Wp = _flipped(np.asarray(weights[cv.name][0], np.float32))[:, :, lg]
    run = R._Run("fp32", np.zeros((1, 1, 1, 1), np.float32), None, "seq", "f32", None, reverse)
    out = np.zeros((len(pix), node.c1 - node.c0))
    out[:, cols] = R._gemm_seq(run, cv.name, xg, Wp, np.zeros(len(lg), np.float32))
    return out


def loss_gradient(y, t, ign, f32=True):
    """compute_loss's gradient of one map tensor (tr_loss): f32(f32(y - t) * f32(2 / numel)), zero where
    ignored; y, t (n, C, h, w), ign (n, h, w).  f32=False: the same in float64 (the CPU chain)."""
    dt = np.float32 if f32 else np.float64
    d = np.asarray(y, dt) - np.asarray(t, dt)
    g = d * dt(2.0 / d.size)
    return np.where(np.asarray(ign, bool)[:, None], dt(0), g)


def map_target(G, node, targets):
    """(C, target tensor) if the node is a stage's map slice (conv5_5 / Mconv7 outputs), else None."""
    if node.kind != "conv" or node.relu or node.c1 - node.c0 not in (40, 20):
        return None
    return (38, targets["pafs"]) if node.c1 - node.c0 == 40 else (19, targets["heat"])


def pool_route(X, dP, last=False):
    """Max-pool 2x2 backward: dP at the first maximum of each window of X in (ky, kx) order
    (tr_pool_bwd), zero elsewhere.  last=True: the last maximum (a defect)."""
    win = np.stack([X[:, :, k >> 1::2, k & 1::2] for k in range(4)])
    best = 3 - np.argmax(win[::-1], axis=0) if last else np.argmax(win, axis=0)
    out = np.zeros(X.shape, dP.dtype)
    for k in range(4):
        out[:, :, k >> 1::2, k & 1::2] = np.where(best == k, dP, 0)
    return out


def node_terms(G, node, T, weights, pix, targets, lowest=0, mutate=None):
    """The addends of the node's gradient at pixels pix, before the producer's mask:
    -> [(consumer conv or None, (P, c1 - c0) float64)].  None: the loss term / a feature-copy gradient,
    taken as the f32 values the device holds (exact addends)."""
    mutate = mutate or {}
    terms = [(cv, input_term(cv, node, T, weights, pix, mutate)) for cv in consumers(G, node, lowest)]
    mt = map_target(G, node, targets)
    if mt is not None:
        C, t = mt
        y = T.act(node.buf)[:, node.c0:node.c0 + C]
        ign = np.zeros_like(targets["ign"]) if mutate.get("no_ignore") else targets["ign"]
        g = np.zeros((len(pix), node.c1 - node.c0))
        g[:, :C] = _at(loss_gradient(y, t, ign, f32=y.dtype == np.float32), pix, 0, C)
        terms.append((None, g))
    if node.kind == "conv" and node.name == "conv4_4_CPM" and lowest < node.layer:
        for s in range(1, 5):
            terms.append((None, _at(T.grad(G.cat[s]), pix, CAT_FEAT, CAT_FEAT + 128).astype(np.float64)))
    return terms


def node_mask(G, node, T, pix, mutate=None):
    """Y > 0 of the producing ReLU at pix (all True where the producer has none)."""
    if not node.relu:
        return np.ones((len(pix), node.c1 - node.c0), bool)
    y = _at(T.act(node.buf), pix, node.c0, node.c1)
    return y >= 0 if (mutate or {}).get("relu_ge") else y > 0


def pooled_by(G, node):
    """Index of the pool that reads the node's buffer, or None."""
    for i, (src, dst) in enumerate(G.pools):
        if node.kind == "conv" and src == node.buf:
            return i
    return None


def conv_input(cv, T):
    """The conv's logical input (n, Ci, h, w) out of its (physical) input buffer."""
    a = T.act(cv.inb)
    if cv.cat:
        m = cat_logical()
        phys = np.empty(cv.ci, np.int64)
        phys[m[m >= 0]] = np.nonzero(m >= 0)[0]
        return a[:, phys]
    return a[:, cv.cin_off:cv.cin_off + cv.ci]


def _wgrad_operands(cv, T):
    dy = T.grad(cv.out)[:, cv.cout_off:cv.cout_off + cv.co]
    n, co, h, w = dy.shape
    g = np.ascontiguousarray(dy.transpose(0, 2, 3, 1)).reshape(n * h * w, co)
    r = cv.k // 2
    xp = np.pad(conv_input(cv, T), ((0, 0), (0, 0), (r, r), (r, r))).transpose(0, 2, 3, 1)

    def shifted(tap):
        return xp[:, tap // cv.k:tap // cv.k + h, tap % cv.k:tap % cv.k + w].reshape(n * h * w, cv.ci)

    return g, shifted


def weight_gradient(cv, T, with_abs=False):
    """-> dW (Co, Ci, k, k), db (Co,) in float64 [, sum |terms| of every dW entry]."""
    g, shifted = _wgrad_operands(cv, T)
    g = g.astype(np.float64)
    taps = cv.k * cv.k
    dW = np.empty((cv.co, cv.ci, taps))
    A = np.empty((cv.co, cv.ci, taps)) if with_abs else None
    for t in range(taps):
        xs = shifted(t).astype(np.float64)
        dW[:, :, t] = g.T @ xs
        if with_abs:
            A[:, :, t] = np.abs(g).T @ np.abs(xs)
    dW = dW.reshape(cv.co, cv.ci, cv.k, cv.k)
    db = g.sum(axis=0)
    return (dW, db, A.reshape(dW.shape)) if with_abs else (dW, db)


def _split_sum(prod, reverse):
    """prod (P, N) float64 addends in raster order -> (N,) the f32 sum tr_wgrad / tr_wreduce form: one
    add per pixel within each split of pps pixels, then the splits in order."""
    P, N = prod.shape
    splits, pps = wgrad_split(P)
    if reverse:
        prod = prod[::-1]
    pad = np.zeros((splits * pps, N))
    pad[:P] = prod  # pixels past the end add nothing (tr_wgrad stages zeros)
    pad = pad.reshape(splits, pps, N)
    acc = np.zeros((splits, N), np.float32)
    for i in range(pps):
        acc = (acc + pad[:, i]).astype(np.float32)
    out = np.zeros(N, np.float32)
    for z in range(splits):
        out = out + acc[z]
    return out.astype(np.float64)


def weight_gradient_seq(cv, T, entries, reverse=False):
    """The yardstick of dW at entries (co, ci, tap) (three equal-length index arrays): float32, one FMA
    per pixel (the product of two f32 is exact in float64, so each step rounds once)."""
    g, shifted = _wgrad_operands(cv, T)
    co, ci, tap = (np.asarray(e, np.int64) for e in entries)
    prod = np.empty((g.shape[0], len(co)))
    for t in np.unique(tap):
        sel = tap == t
        prod[:, sel] = g[:, co[sel]].astype(np.float64) * shifted(int(t))[:, ci[sel]].astype(np.float64)
    return _split_sum(prod, reverse)


def bias_gradient_seq(cv, T, reverse=False):
    """The yardstick of db (all channels): plain f32 adds in tr_wgrad's order."""
    g, _ = _wgrad_operands(cv, T)
    return _split_sum(np.asarray(g, np.float32).astype(np.float64), reverse)


def wgrad_entries(ideal, sum_abs, rng, n=384):
    """(co, ci, tap) of the weight-gradient entries the yardstick is evaluated at: a third with the
    largest sum |terms| (the running sum's error grows with its partial sums), a third with the
    largest |ideal| (where the error shows), a third random -- layer_ref.yardstick_pixels's argument
    for entries.  A pure function of the ideal."""
    flat = ideal.reshape(ideal.shape[0], ideal.shape[1], -1)
    size = flat.size
    n = min(n, size)
    third = (n + 2) // 3
    a = np.argsort(-sum_abs.reshape(-1), kind="stable")[:third]
    b = np.argsort(-np.abs(flat).reshape(-1), kind="stable")[:third]
    top = np.unique(np.concatenate([a, b]))
    rest = np.setdiff1d(np.arange(size), top)
    extra = rng.choice(rest, min(max(n - len(top), 0), len(rest)), replace=False) if len(rest) else rest
    return np.unravel_index(np.concatenate([top, extra]).astype(np.int64), flat.shape)


# ---- the whole step in one precision (the CPU wiring test) ----
def forward(G, weights, x, dtype=np.float64):
    """Every activation buffer of the step, physical layout, in `dtype`."""
    n, _, h, w = x.shape
    T = Tensors()
    for i, (_, ch, div) in enumerate(G.bufs):
        T._a[i] = np.zeros((n, ch, h // div, w // div), dtype)
    T._a[0][:, :3] = x
    pool_of = dict(G.pools)
    for cv in G.convs:
        X = conv_input(cv, T)
        W, b = (np.asarray(a, dtype) for a in weights[cv.name])
        _, _, hh, ww = X.shape
        xg = _gather(X, R.all_pixels(n, hh, ww), cv.k)
        y = xg.reshape(len(xg), -1) @ W.reshape(cv.co, cv.ci, -1).transpose(2, 1, 0).reshape(-1, cv.co) + b
        y = R.to_nchw(y, n, hh, ww)
        T._a[cv.out][:, cv.cout_off:cv.cout_off + cv.co] = np.maximum(y, 0) if cv.relu else y
        if cv.out in pool_of:
            a = T._a[cv.out]
            T._a[pool_of[cv.out]] = np.maximum(np.maximum(a[:, :, 0::2, 0::2], a[:, :, 0::2, 1::2]),
                                               np.maximum(a[:, :, 1::2, 0::2], a[:, :, 1::2, 1::2]))
        if cv.name == "conv4_4_CPM":
            for s in range(1, 5):
                T._a[G.cat[s]][:, CAT_FEAT:CAT_FEAT + 128] = T._a[G.cat[0]][:, CAT_FEAT:CAT_FEAT + 128]
    return T


def backward(G, weights, T, targets):
    """Chains the per-node ideals from the loss down, each fed its own output: fills T's gradient
    buffers and returns {layer name: (dW, db)}."""
    for i in range(len(G.bufs)):
        T._g[i] = np.zeros_like(T._a[i])
    n = T._a[0].shape[0]
    grads = {}
    for key in G.order:
        node = G.nodes[key]
        _, _, h, w = T._a[node.buf].shape
        pix = R.all_pixels(n, h, w)
        pi = pooled_by(G, node)
        if pi is not None:
            g = pool_route(T._a[node.buf], T._g[G.pools[pi][1]])
            g = np.where(T._a[node.buf] > 0, g, 0)
        else:
            total = sum(v for _, v in node_terms(G, node, T, weights, pix, targets))
            g = R.to_nchw(np.where(node_mask(G, node, T, pix), total, 0.0), n, h, w)
        T._g[node.buf][:, node.c0:node.c1] = g
        if node.kind == "conv":
            grads[node.name] = weight_gradient(G.convs[node.layer], T)
    return grads
