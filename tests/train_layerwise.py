"""Helpers of the training tests (a plain module: no fixtures, no collection hooks): the float64 torch
autograd restatement of one training iteration, the seeded data, the configurations of
tests/test_gpu_train_layerwise.py and the comparison of one backward launch with oracle/train_ref.py
(the tolerances live here, so the CPU tests of tests/test_train_ref.py judge the same ones)."""
import json
import os

import numpy as np

import layerwise as LW
from oracle import layer_ref as R
from oracle import train_ref as TR

# name: (n, h, w), settings.  frozen: the VGG_FROZEN layers disabled (lowest = 10); ties: conv3_4's
# weights zero and bias 0.5, so every window of pool3 ties at a positive value.
CONFIGS = {
    # today's shape: every weight-gradient split full; tile widths 16 (w 48, 12, 6) and 32 (w 24)
    "2x64x48": dict(shape=(2, 64, 48)),
    # 1600 px: 3 splits of 544, the last 512; weight-gradient tails 100 % 16 = 4, 25 % 16 = 9; 25 < 32
    # pixels for the 1x1 input-gradient convs
    "1x40x40": dict(shape=(1, 40, 40)),
    # frames of 15 and 60 pixels: 16-pixel steps and 32-pixel blocks cross frame borders; widths 5, 10, 20
    "3x24x40": dict(shape=(3, 24, 40)),
    # 32832 = 64 x 513 px: 64 splits of 528, the 64th empty, the 63rd 96 px; widths 152 / 76 / 38 / 19
    "3x72x152": dict(shape=(3, 72, 152)),
    "2x64x48-frozen": dict(shape=(2, 64, 48), frozen=True),
    "3x24x40-ties": dict(shape=(3, 24, 40), ties=True),
}
R_F32 = 2.0 ** -23


def torch_step(W, x, pafs_t, heat_t, ignore):
    """(losses[12], grads {layer: (gW, gb)}) in float64: train_coco_pose_estimation.py:42-123
    (CocoPoseNet.__call__ with every stage's maps, compute_loss with the ignore mask, backward)."""
    import torch
    tf = torch.nn.functional
    P = {k: (torch.tensor(w, dtype=torch.float64, requires_grad=True),
             torch.tensor(b, dtype=torch.float64, requires_grad=True)) for k, (w, b) in W.items()}

    def conv(name, h, act=True):
        w, b = P[name]
        y = tf.conv2d(h, w, b, padding=w.shape[2] // 2)
        return torch.relu(y) if act else y

    h = torch.tensor(x, dtype=torch.float64)
    for blk in (("conv1_1", "conv1_2"), ("conv2_1", "conv2_2"), ("conv3_1", "conv3_2", "conv3_3", "conv3_4")):
        for n in blk:
            h = conv(n, h)
        h = tf.max_pool2d(h, 2)
    for n in ("conv4_1", "conv4_2", "conv4_3_CPM", "conv4_4_CPM"):
        h = conv(n, h)
    feat = h
    outs = []
    h1, h2 = feat, feat
    for i in (1, 2, 3, 4):
        h1 = conv("conv5_%d_CPM_L1" % i, h1)
        h2 = conv("conv5_%d_CPM_L2" % i, h2)
    h1, h2 = conv("conv5_5_CPM_L1", h1, False), conv("conv5_5_CPM_L2", h2, False)
    outs.append((h1, h2))
    for s in range(2, 7):
        cat = torch.cat((h1, h2, feat), 1)
        t1, t2 = cat, cat
        for i in range(1, 7):
            t1 = conv("Mconv%d_stage%d_L1" % (i, s), t1)
            t2 = conv("Mconv%d_stage%d_L2" % (i, s), t2)
        h1, h2 = conv("Mconv7_stage%d_L1" % s, t1, False), conv("Mconv7_stage%d_L2" % s, t2, False)
        outs.append((h1, h2))
    pt = torch.tensor(pafs_t, dtype=torch.float64)
    ht = torch.tensor(heat_t, dtype=torch.float64)
    m = torch.tensor(ignore.astype(bool))[:, None]
    total = 0
    losses = []
    for py, hy in outs:  # compute_loss: masked targets take the prediction's value
        tp = torch.where(m.expand_as(py), py.detach(), pt)
        th = torch.where(m.expand_as(hy), hy.detach(), ht)
        lp, lh = ((py - tp) ** 2).mean(), ((hy - th) ** 2).mean()
        losses += [float(lp), float(lh)]
        total = total + lp + lh
    total.backward()
    return np.array(losses), {k: (w.grad.numpy(), b.grad.numpy()) for k, (w, b) in P.items()}


def hook_multipliers():
    with open(os.path.join(os.path.dirname(__file__), "golden", "train", "host_schedule.json")) as f:
        return json.load(f)["hooks"][0]["multiplier_by_layer"]


def data(n, h, w, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.5, 0.5, (n, 3, h, w)).astype(np.float32)
    pt = rng.uniform(-1, 1, (n, 38, h // 8, w // 8)).astype(np.float32)
    ht = rng.uniform(0, 1, (n, 19, h // 8, w // 8)).astype(np.float32)
    ig = (rng.random((n, h // 8, w // 8)) < 0.2).astype(np.uint8)
    return x, pt, ht, ig


def config_weights(cfg, weights):
    """The configuration's weights: `weights`, with conv3_4 made constant 0.5 for the tie case."""
    if not cfg.get("ties"):
        return weights
    W = dict(weights)
    w, b = W["conv3_4"]
    W["conv3_4"] = (np.zeros_like(w), np.full_like(b, 0.5))
    return W


def check_input_gradient(G, node, T, weights, targets, n_batch, lowest=0, mutate=None, seq_reverse=False, got=None):
    """One node's gradient against its reference at the checked pixels (layerwise.checked_pixels: all
    of them up to 4096 per launch), all channels:

        |g - ideal| <= 2 sum_consumers e_seq + k 2^-23 sum |terms|

    e_seq per consumer conv = the largest |seq - term| over layer_ref.yardstick_pixels of that term, k =
    the f32 additions that round: the addends go one after the other into a zeroed buffer, so the first
    is exact and k = addends - 1.  Elements the producer's ReLU masks are held to exactly 0.  got: the
    gradient to judge (default: T's own); mutate: a defect put into the *judged* value (the CPU
    sensitivity tests) -- then `got` is the mutated ideal."""
    _, _, h, w = T.act(node.buf).shape
    rng = np.random.default_rng(1000 + (node.layer if node.layer is not None else 500 + node.buf))
    pix = LW.checked_pixels(n_batch, n_batch, h, w, rng)
    terms = TR.node_terms(G, node, T, weights, pix, targets, lowest)
    total = sum(v for _, v in terms) if terms else np.zeros((len(pix), node.c1 - node.c0))
    sum_abs = sum(np.abs(v) for _, v in terms) if terms else np.zeros_like(total)
    mask = TR.node_mask(G, node, T, pix)
    ideal = np.where(mask, total, 0.0)
    e_seq = 0.0
    for cv, v in terms:
        if cv is None:
            continue
        sample = R.yardstick_pixels(v, cv.k, rng)
        seq = TR.input_term_seq(cv, node, T, weights, pix[sample], reverse=seq_reverse)
        e_seq += float(np.abs(seq - v[sample]).max())
    k = max(len(terms) - 1, 0)
    tol = 2.0 * e_seq + k * R_F32 * sum_abs
    if mutate is not None:
        mt = TR.node_terms(G, node, T, weights, pix, targets, lowest, mutate)
        gv = np.where(TR.node_mask(G, node, T, pix, mutate), sum(v for _, v in mt), 0.0)
    elif got is not None:
        gv = got
    else:
        gv = TR._at(T.grad(node.buf), pix, node.c0, node.c1).astype(np.float64)
    err = np.abs(gv - ideal)
    masked_nonzero = int(np.count_nonzero(gv[~mask]))
    rel = err / np.maximum(tol, 1e-300)
    rest = k * R_F32 * sum_abs
    need = float(((err - rest) / e_seq).max()) if e_seq > 0 else (0.0 if not err.any() else float("inf"))
    i, c = np.unravel_index(int(np.argmax(rel)), rel.shape)
    return dict(max_err=float(err.max()), e_seq=e_seq, ratio=float(err.max() / e_seq) if e_seq > 0 else 0.0, need=need,
                worst=float(rel[i, c]), at=(int(pix[i, 0]), int(c), int(pix[i, 1]), int(pix[i, 2])), n=int(err.size),
                terms=len(terms), bad=int((err > tol).sum()), masked_nonzero=masked_nonzero, pix=pix,
                ideal=ideal, tol=tol, mask=mask)


def check_weight_gradient(cv, T, got_W, got_b, seq_reverse=False):
    """One layer's dW and db against their reference, every entry:

        |dW - ideal| <= 2 e_seq + 2^-23 |ideal|

    e_seq = the largest |seq - ideal| over train_ref.wgrad_entries (dW) / over all channels (db)."""
    dW, db, A = TR.weight_gradient(cv, T, with_abs=True)
    rng = np.random.default_rng(2000 + cv.layer)
    ent = TR.wgrad_entries(dW, A, rng)
    flat = dW.reshape(cv.co, cv.ci, -1)
    e_w = float(np.abs(TR.weight_gradient_seq(cv, T, ent, reverse=seq_reverse) - flat[ent]).max())
    e_b = float(np.abs(TR.bias_gradient_seq(cv, T, reverse=seq_reverse) - db).max())
    out = {}
    for key, got, want, e in (("W", got_W, dW, e_w), ("b", got_b, db, e_b)):
        err = np.abs(np.asarray(got, np.float64) - want)
        tol = 2.0 * e + R_F32 * np.abs(want)
        need = float(((err - R_F32 * np.abs(want)) / e).max()) if e > 0 else (0.0 if not err.any() else float("inf"))
        out[key] = dict(max_err=float(err.max()), e_seq=e, ratio=float(err.max() / e) if e > 0 else 0.0, need=need,
                        worst=float((err / np.maximum(tol, 1e-300)).max()), n=int(err.size), bad=int((err > tol).sum()),
                        ideal=want, tol=tol)
    return out


def line(kind, config, name, r):
    return "LAYERWISE %s %s %s: max|err| %.3e e_seq %.3e ratio %.2f need %.2f worst err/tol %.3f (%d outputs)" % (
        config, kind, name, r["max_err"], r["e_seq"], r["ratio"], r["need"], r["worst"], r["n"])
