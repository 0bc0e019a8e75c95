"""The two command-line ends of the overlay: ``--overlay`` of the detector CLI (the network's maps over
the frame, through overlay_staged) and ``--dump-samples`` of the trainer (the reference loader's viewer
picture, coco_data_loader.py:372-384, through make_labels and overlay_labels)."""
import json
import os

import numpy as np
import pytest

from conftest import people_image, pkg_module

pytestmark = pytest.mark.gpu

HUE_MARGIN = 1e-9  # tests/test_gpu_overlay.py


def margin_ok(ov, hw, pafs):
    return ov.hue_margin(ov.mix_pafs_np(ov.resize_linear_f32_np(pafs, *hw))) > HUE_MARGIN


def test_cli_overlay_writes_the_maps_over_the_frame(tmp_path, pkg, rand_weights):
    from PIL import Image
    W, D, ov = pkg_module("weights"), pkg_module("draw"), pkg_module("overlay")
    wpath, ipath = str(tmp_path / "w.npz"), str(tmp_path / "in.png")
    W.save_npz(wpath, rand_weights)
    img = people_image()
    Image.fromarray(img[:, :, ::-1]).save(ipath)
    det = pkg.PoseDetector("posenet", model=rand_weights)
    det(img)
    pafs, heat = det._ctx.fetch_maps(0, 1)
    assert margin_ok(ov, img.shape[:2], pafs[0])
    for layers, want in (("pafs,heatmaps", ov.overlay_np(img, pafs[0], heat[0, :18])), ("pafs", ov.overlay_np(img, pafs[0]))):
        out, shown = str(tmp_path / "result.png"), str(tmp_path / ("maps_%s.png" % layers.replace(",", "_")))
        assert D.main(["posenet", wpath, "--img", ipath, "--out", out, "--overlay", layers, "--overlay-out", shown]) == 0
        assert np.array_equal(D.read_bgr(shown), want) and (want != img).any()
        assert os.path.exists(out)
    with pytest.raises(SystemExit):
        D.main(["posenet", wpath, "--img", ipath, "--overlay", "pafs,mask"])


def test_train_dump_samples_writes_the_viewer_picture(tmp_path):
    T, L, D, ov = pkg_module("train"), pkg_module("labels"), pkg_module("draw"), pkg_module("overlay")
    n, insize, seed, people = 2, 48, 7, 2
    common = ["--batchsize", str(n), "--iteration", "2", "--insize", str(insize), "--seed", str(seed), "--people", str(people)]
    logs = {}
    for data in ("poses", "samples"):
        for dump in (False, True):
            out, pics = str(tmp_path / (data + str(dump))), str(tmp_path / (data + "_pics"))
            extra = ["--dump-samples", pics, "--dump-count", "3"] if dump else []
            assert T.main(["--data", data, "--out", out] + common + extra) == 0
            logs[data, dump] = [(e["main/loss"], e["main/paf"], e["main/heat"]) for e in json.load(open(os.path.join(out, "log")))]
        assert logs[data, True] == logs[data, False]  # looking does not change the training
        names = sorted(os.listdir(pics))
        assert names == ["sample_%04d.png" % k for k in range(3)]  # the first batch and one of the second
        for name in names:
            pic = D.read_bgr(os.path.join(pics, name))
            assert pic.shape == (insize, 2 * insize, 3) and (pic[:, :insize] != pic[:, insize:]).any()
    # --data poses draws its batches from default_rng(seed): the first one again, through the statement
    rng = np.random.default_rng(seed)
    imgs = rng.integers(0, 256, (n, insize, insize, 3), dtype=np.uint8)
    poses = T.synthetic_poses(rng, n, insize, insize, people)
    mask = rng.random((n, insize, insize)) < 0.0005
    pafs, heat, ign = L.make_labels(poses, insize, insize, mask)
    for i in range(n):
        assert margin_ok(ov, (insize, insize), pafs[i])
        want = np.hstack((imgs[i], ov.overlay_labels_np(imgs[i], pafs[i], heat[i], ign[i])))
        assert np.array_equal(D.read_bgr(str(tmp_path / "poses_pics" / ("sample_%04d.png" % i))), want)
    with pytest.raises(SystemExit):
        T.main(["--data", "maps", "--dump-samples", str(tmp_path / "x")] + common)
