"""Augmentation on the GPU (op_augment, csrc/augment.hip) against augment.py's augment_np, bit for
bit: the pixel path is integer arithmetic plus f32 statements of one explicitly rounded operation
each, so no tolerance applies.  augment_np itself is held to the reference's crop / flip and to its
stated arithmetic in test_augment_host.py.

The LDS path and the global-memory path.  A 16 x 16 tile's source box under a pure rotation is at
most 16 (|cos| + |sin|) + 4 <= 27 pixels a side, within the kernel's 32 x 32 staging box at every
angle, so no rotation plan can reach the fallback; a minifying matrix (a quarter-scale forward map:
a tile spans 64 source pixels) does, and the C ABI accepts any finite matrix.  The path test runs a
45 degree plan (the widest rotated box) and that minifying plan and prints both counts."""
import glob
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN, pkg_module

pytestmark = pytest.mark.gpu

SOURCES = {"a": (96, 128), "b": (75, 101)}


@pytest.fixture(scope="module")
def aug():
    return pkg_module("augment")


def fixture_plan(aug, k):
    """(plan, poses_in) of tests/golden/augment/plan_<k>.npz, drawn as the host test pins it."""
    r = np.load(os.path.join(GOLDEN, "augment", "plan_%d.npz" % k))
    seed = int(r["seed"])
    plan, _ = aug.draw_plan(r["poses_in"], int(r["h"]), int(r["w"]), int(r["insize"]), random.Random(seed),
                            np.random.RandomState(seed))
    return plan


def hand_plan(aug, h, w, rw, rh, degree, insize, center=None, colour=None, flip=False):
    R, bw, bh = aug.rotate_geometry(rw, rh, degree)
    center = (bw // 2, bh // 2) if center is None else center
    return aug.AugmentPlan(h=h, w=w, rw=rw, rh=rh, degree=degree, R=R, bw=bw, bh=bh, colour=colour, flip=flip,
                           insize=insize, **aug.crop_window(center, insize, bw, bh))


def identity_plan(aug, h, w, insize, center, flip=False):
    """Same-size resize, degree 0, crop centred at ``center`` (test_augment_host.py's)."""
    return aug.AugmentPlan(h=h, w=w, rw=w, rh=h, degree=0.0, R=aug.rotation_matrix((w / 2, h / 2), 0.0), bw=w, bh=h,
                           colour=None, flip=flip, insize=insize, **aug.crop_window(center, insize, w, h))


def sample_for(plan, seed, with_mask=True):
    rng = np.random.default_rng([seed, plan.h, plan.w])
    img = rng.integers(0, 256, (plan.h, plan.w, 3), dtype=np.uint8)
    mask = np.zeros((plan.h, plan.w), bool)
    mask[plan.h // 4:plan.h // 2, plan.w // 3:2 * plan.w // 3] = True
    mask |= rng.random((plan.h, plan.w)) < 0.02
    return img, (mask if with_mask else None)


@pytest.fixture(scope="module")
def batches(aug):
    """The two calls of the six-sample batch: {insize: (plans, imgs, masks)}; 96x128 and 75x101
    sources in both; three fixture plans and three hand-made ones."""
    p64 = [fixture_plan(aug, 0), fixture_plan(aug, 3), hand_plan(aug, 75, 101, 90, 70, 90.0, 64, colour=(4, -20, 11))]
    miss = hand_plan(aug, 96, 128, 100, 80, 10.0, 64, flip=True)
    miss.x1, miss.x2, miss.x_from, miss.x_to = 5, 4, 0, -1  # the window misses the rotated image: nothing copied
    p64.append(miss)
    p160 = [fixture_plan(aug, 11), hand_plan(aug, 75, 101, 150, 120, 180.0, 160, colour=(-10, 40, -30), flip=True)]
    assert {(p.h, p.w) for p in p64} == {(p.h, p.w) for p in p160} == set(SOURCES.values())
    out = {}
    for insize, plans in ((64, p64), (160, p160)):
        pairs = [sample_for(p, 10 * insize + i) for i, p in enumerate(plans)]
        out[insize] = (plans, [a for a, _ in pairs], [m for _, m in pairs])
    return out


@pytest.fixture(scope="module")
def want(aug, batches):
    """augment_np of every sample, computed once."""
    return {insize: [aug.augment_np(i, m, p) for p, i, m in zip(plans, imgs, masks)]
            for insize, (plans, imgs, masks) in batches.items()}


@pytest.fixture(scope="module")
def got(aug, batches):
    return {insize: aug.augment(imgs, masks, plans) for insize, (plans, imgs, masks) in batches.items()}


def test_last_ms_needs_a_call(aug, lib):
    """OP_ERR_STATE on a device index no call has completed on; positive after a call."""
    with pytest.raises(RuntimeError):
        aug.last_ms(63)
    with pytest.raises(RuntimeError):
        aug.last_paths(63)
    plan = hand_plan(aug, 20, 30, 30, 20, 5.0, 32)
    aug.augment([sample_for(plan, 1)[0]], None, [plan])
    ms = aug.last_ms(0)
    print("op_augment_last_ms", ms)
    assert ms > 0


def test_batch_equals_augment_np(batches, want, got):
    for insize, (plans, imgs, masks) in batches.items():
        oimg, omask = got[insize]
        assert oimg.shape == (len(plans), insize, insize, 3) and omask.shape == (len(plans), insize, insize)
        for f, (wi, wm) in enumerate(want[insize]):
            nbad = int((oimg[f] != wi).sum())
            print("insize %d sample %d: %d differing bytes, mask %d differing" % (insize, f, nbad, int((omask[f] != wm).sum())))
            assert np.array_equal(oimg[f], wi), (insize, f)
            assert np.array_equal(omask[f], wm), (insize, f)
    # the case that nothing is copied: all pad, nothing ignored; and the others are not trivial
    assert (got[64][0][3] == 127).all() and not got[64][1][3].any()
    for insize in batches:
        for f, (wi, wm) in enumerate(want[insize]):
            if not (insize == 64 and f == 3):
                assert len(np.unique(wi)) > 50 and wm.any() and not wm.all(), (insize, f)


def test_batch_equals_samples_run_singly(aug, batches, got):
    for insize, (plans, imgs, masks) in batches.items():
        for f, plan in enumerate(plans):
            oimg, omask = aug.augment([imgs[f]], [masks[f]], [plan])
            lds, fallback = aug.last_paths(0)
            print("insize %d sample %d: %d pixels from LDS, %d from global memory" % (insize, f, lds, fallback))
            assert np.array_equal(oimg[0], got[insize][0][f]) and np.array_equal(omask[0], got[insize][1][f])
            inside = 0 if plan.window_empty() else (plan.x_to - plan.x_from + 1) * (plan.y_to - plan.y_from + 1)
            assert lds + fallback == inside


def test_both_paths_are_exercised(aug):
    wide = hand_plan(aug, 96, 128, 128, 96, 45.0, 64)
    R = np.array([[0.25 * np.cos(0.3), 0.25 * np.sin(0.3), 6.0], [-0.25 * np.sin(0.3), 0.25 * np.cos(0.3), 14.0]])
    mini = aug.AugmentPlan(h=96, w=128, rw=128, rh=96, degree=0.0, R=R, bw=40, bh=36, colour=None, flip=False, insize=64,
                           **aug.crop_window((20, 18), 64, 40, 36))
    counts = []
    for name, plan in (("45 degrees", wide), ("quarter scale", mini)):
        img, mask = sample_for(plan, 77)
        oimg, omask = aug.augment([img], [mask], [plan])
        counts.append(aug.last_paths(0))
        print("%s: %d pixels from LDS, %d from global memory" % ((name,) + counts[-1]))
        wi, wm = aug.augment_np(img, mask, plan)
        assert np.array_equal(oimg[0], wi) and np.array_equal(omask[0], wm), name
    assert counts[0][0] > 0 and counts[0][1] == 0
    assert counts[1][1] > 0


def test_null_masks(aug, batches, got):
    plans, imgs, masks = batches[64]
    oimg, omask = aug.augment(imgs, None, plans)
    assert np.array_equal(oimg, got[64][0]) and not omask.any()
    some = [masks[0], None] + masks[2:]
    oimg, omask = aug.augment(imgs, some, plans)
    assert np.array_equal(oimg, got[64][0])
    assert not omask[1].any() and np.array_equal(np.delete(omask, 1, axis=0), np.delete(got[64][1], 1, axis=0))


def test_cropflip_fixtures_on_the_device(aug):
    """The device twin of the identity test: the reference's own random_crop_img / flip_img outputs."""
    by_insize = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN, "augment", "cropflip_*.npz"))):
        r = np.load(path)
        by_insize.setdefault(int(r["insize"]), []).append(r)
    assert sorted(by_insize) == [64, 160]
    for insize, recs in by_insize.items():
        plans, imgs, masks, wants = [], [], [], []
        for r in recs:
            h, w = r["mask"].shape
            offset = r["poses_in"][0, 0, :2] - r["crop_poses"][0, 0, :2]
            for flip in (False, True):
                plans.append(identity_plan(aug, h, w, insize, offset + insize // 2 - 1, flip=flip))
                imgs.append(r["img"])
                masks.append(r["mask"])
                wants.append((r["flip_img"], r["flip_mask"]) if flip else (r["crop_img"], r["crop_mask"]))
        oimg, omask = aug.augment(imgs, masks, plans)
        for f, (wi, wm) in enumerate(wants):
            assert np.array_equal(oimg[f], wi) and np.array_equal(omask[f], wm), (insize, f)


def test_update_samples_equals_update_poses_on_the_augmented_batch(aug, lib, rand_weights):
    """Same shape as test_step_poses_equals_step_on_device_made_labels: losses, gradients and
    weights bit for bit."""
    train = pkg_module("train")
    n, insize = 2, 48
    samples = train.synthetic_samples(np.random.default_rng(3), n, people=2, sizes=((60, 80), (75, 101)))
    out = []
    for chained in (True, False):
        up = train.Updater(n, insize, insize, model=rand_weights)
        try:
            py, npr = random.Random(5), np.random.RandomState(5)
            if chained:
                loss = up.update_samples(samples, py, npr)
            else:
                imgs, poses, mask = aug.augment_batch(samples, insize, py, npr)
                assert imgs.shape == (n, insize, insize, 3) and len(np.unique(imgs)) > 50
                loss = up.update_poses(imgs, poses, mask)
            out.append((loss, up.grads(), up.weights()))
        finally:
            up.ctx.close()
    (l0, g0, w0), (l1, g1, w1) = out
    assert l0[0] > 0 and l0 == l1
    for name in g0:
        for k in (0, 1):
            assert np.array_equal(g0[name][k], g1[name][k]), name
            assert np.array_equal(w0[name][k], w1[name][k]), name


def test_cli_samples_is_reproducible(tmp_path):
    """--data samples: the same seed gives the same losses."""
    import json
    train = pkg_module("train")
    logs = []
    for run in ("a", "b"):
        out = str(tmp_path / run)
        assert train.main(["--data", "samples", "--batchsize", "2", "--iteration", "2", "--insize", "48", "--seed", "7",
                           "--people", "2", "--out", out]) == 0
        logs.append([(e["main/loss"], e["main/paf"], e["main/heat"]) for e in json.load(open(os.path.join(out, "log")))])
        assert all("augment_ms" in e and e["augment_ms"] > 0 for e in json.load(open(os.path.join(out, "log"))))
    assert len(logs[0]) == 2 and logs[0] == logs[1]
