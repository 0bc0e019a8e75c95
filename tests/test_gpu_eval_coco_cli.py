"""``python -m <package>.eval_coco`` on the GPU: a plumbing run with random weights on a tiny
annotations file (the results file against ``PoseDetector`` + ``to_coco`` on the same frames), and
``--results-in`` on a results file made from the ground truths."""
import json

import numpy as np
import pytest

import keypoint_cases as cases
from conftest import pkg_module

pytestmark = pytest.mark.gpu

SIZES = {1: (96, 128), 2: (128, 96), 5: (96, 128)}  # image id -> (h, w): two sizes


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """Three images of two sizes, image 2 without persons, one crowd annotation in image 5."""
    from PIL import Image
    root = tmp_path_factory.mktemp("coco")
    rng = np.random.default_rng(41)
    images, anns, frames = [], [], {}
    for img_id, (h, w) in SIZES.items():
        name = "%012d.png" % img_id
        frames[img_id] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)  # BGR
        Image.fromarray(np.ascontiguousarray(frames[img_id][:, :, ::-1])).save(str(root / name))
        images.append({"id": img_id, "height": h, "width": w, "file_name": name})
    for img_id, size, visible, crowd in ((1, 60.0, 17, 0), (1, 50.0, 9, 0), (5, 70.0, 12, 0), (5, 80.0, 0, 1)):
        kp = cases.person(rng, 64, 48, size, visible).round()
        anns.append({"id": len(anns) + 1, "image_id": img_id, "category_id": 1, "iscrowd": crowd,
                     "keypoints": [int(v) for v in kp.ravel()], "num_keypoints": visible, "area": size * size / 2,
                     "bbox": [64 - size / 2, 48 - size / 2, size, size]})
    path = root / "person_keypoints_tiny.json"
    path.write_text(json.dumps({"images": images[::-1], "annotations": anns, "categories": [{"id": 1, "name": "person"}]}))
    return {"root": root, "annotations": str(path), "frames": frames, "anns": anns}


def _lines(out):
    return [l for l in out.splitlines() if l.startswith(" Average ")]


def test_plumbing_run_with_random_weights(dataset, rand_weights, capsys, tmp_path):
    K, cli = pkg_module("keypoint_eval"), pkg_module("eval_coco")
    out = tmp_path / "results.json"
    assert cli.main(["--annotations", dataset["annotations"], "--images", str(dataset["root"]), "--random-weights",
                     "--batch", "2", "--results", str(out)]) == 0
    lines = _lines(capsys.readouterr().out)
    assert len(lines) == 10 and lines[0].startswith(" Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets= 20 ] = ")
    entries = json.loads(out.read_text())
    # the same frames through PoseDetector's staged step, bucketed by size as the tool buckets them
    det = pkg_module("pose_detector").PoseDetector("posenet", model=rand_weights, max_batch=2)
    want = {}
    for ids in ([1, 5], [2]):
        n = det.run_staged(np.stack([dataset["frames"][i] for i in ids]))
        det.staged_context().synchronize()
        for i, (poses, scores, _) in zip(ids, det.staged_context().fetch_results(0, n)):
            want[i] = K.results_json(i, poses, scores)
    assert entries == want[1] + want[2] + want[5]
    for e in entries:
        assert e["category_id"] == 1 and len(e["keypoints"]) == 51 and e["image_id"] in SIZES


def test_results_in_scores_a_results_file(dataset, capsys, tmp_path):
    cli = pkg_module("eval_coco")
    entries = [{"image_id": a["image_id"], "category_id": 1, "keypoints": a["keypoints"], "score": 1.0 + a["id"]}
               for a in dataset["anns"] if not a["iscrowd"]]
    path = tmp_path / "from_gt.json"
    path.write_text(json.dumps(entries))
    assert cli.main(["--annotations", dataset["annotations"], "--results-in", str(path)]) == 0
    lines = _lines(capsys.readouterr().out)
    assert len(lines) == 10
    # areas 1800, 1250 and 2450: all in "medium", none in "large"
    values = [l.rsplit("= ", 1)[1] for l in lines]
    assert values == ["1.000", "1.000", "1.000", "1.000", "-1.000", "1.000", "1.000", "1.000", "1.000", "-1.000"], values
