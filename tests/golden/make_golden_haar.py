"""Writes the hand-made cascade fixtures of tests/golden/haar (the real cascade,
haarcascade_frontalface_alt.xml.gz, is the reference's file, gzip -9 -n of its unchanged bytes):

  tiny_cascade.xml     two stages (3 + 4 stumps) on a 6 x 5 window, one stump with a three-rect feature.
                       Every feature's weighted areas cancel, so on noise a stump votes about half the
                       time: stage 0 wants two of three votes (about half the windows pass), stage 1's
                       leaves 1, 1, 1, 1.5 against 2.25 pass half of those again (about a quarter
                       overall) -- many survivors for the skip rule, the compaction and the cap.
  refuse_*.xml         one file per ValueError of haar.load_cascade.

  crop_face_ref.json   with --reference DIR (the build container only): what the reference's own
                       camera_face_demo.crop_face returns for seeded rects on a seeded frame -- its
                       (left, top), the square's side and a digest of its bytes.  The function is cut
                       out of the file (importing the file needs cv2 and chainer) and run unmodified
                       with the reference's own face_crop_scale.

Run from the repository root: python tests/golden/make_golden_haar.py [--reference DIR]
"""
import ast
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "haar")

# (rects as x y w h weight, threshold, left, right)
TINY_FEATURES = [
    [(0, 0, 6, 5, -1.0), (0, 0, 3, 5, 2.0)],
    [(0, 0, 6, 5, -1.0), (0, 0, 6, 2, 2.5)],
    [(0, 0, 6, 5, -1.0), (0, 0, 2, 5, 1.5), (4, 0, 2, 5, 1.5)],
    [(1, 1, 4, 3, -1.0), (1, 1, 2, 3, 2.0)],
    [(0, 0, 6, 4, -1.0), (0, 0, 6, 2, 2.0)],
    [(0, 0, 4, 4, -1.0), (0, 0, 2, 2, 2.0), (2, 2, 2, 2, 2.0)],
    [(2, 1, 4, 4, -1.0), (2, 1, 4, 2, 2.0)],
]
TINY_STAGES = [
    (1.5, [(0, 0.0125, 0.0, 1.0), (1, -0.02, 1.0, 0.0), (2, 0.005, 0.0, 1.0)]),
    (2.25, [(3, 0.01, 0.0, 1.0), (4, -0.015, 1.0, 0.0), (5, 0.0, 0.0, 1.0), (6, 0.02, 1.5, 0.0)]),
]


def cascade_xml(width, height, features, stages, stage_type="BOOST", feature_type="HAAR", tilted=(), nodes=None):
    out = ["<?xml version=\"1.0\"?>", "<opencv_storage>",
           "<cascade type_id=\"opencv-cascade-classifier\"><stageType>%s</stageType>" % stage_type,
           "  <featureType>%s</featureType>" % feature_type, "  <height>%d</height>" % height, "  <width>%d</width>" % width,
           "  <stageParams>", "    <maxWeakCount>%d</maxWeakCount></stageParams>" % max(len(s[1]) for s in stages),
           "  <featureParams>", "    <maxCatCount>0</maxCatCount></featureParams>",
           "  <stageNum>%d</stageNum>" % len(stages), "  <stages>"]
    for thr, stumps in stages:
        out += ["    <_>", "      <maxWeakCount>%d</maxWeakCount>" % len(stumps),
                "      <stageThreshold>%r</stageThreshold>" % thr, "      <weakClassifiers>"]
        for f, t, left, right in stumps:
            out += ["        <_><internalNodes>%s</internalNodes><leafValues>%r %r%s</leafValues></_>"
                    % (nodes or "0 -1 %d %r" % (f, t), left, right, " 0.5" if nodes else "")]
        out += ["      </weakClassifiers></_>"]
    out += ["  </stages>", "  <features>"]
    for i, rects in enumerate(features):
        out += ["    <_><rects>%s</rects><tilted>%d</tilted></_>"
                % ("".join("<_>%d %d %d %d %r</_>" % r for r in rects), 1 if i in tilted else 0)]
    out += ["  </features></cascade>", "</opencv_storage>", ""]
    return "\n".join(out)


OLD_FORMAT = """<?xml version="1.0"?>
<opencv_storage>
<haarcascade_tiny type_id="opencv-haar-classifier">
  <size>6 5</size>
  <stages>
    <_>
      <trees>
        <_>
          <_>
            <feature>
              <rects>
                <_>0 0 6 5 -1.</_>
                <_>0 0 3 5 2.</_></rects>
              <tilted>0</tilted></feature>
            <threshold>0.0125</threshold>
            <left_val>0.</left_val>
            <right_val>1.</right_val></_></_></trees>
      <stage_threshold>0.5</stage_threshold>
      <parent>-1</parent>
      <next>-1</next></_></stages></haarcascade_tiny>
</opencv_storage>
"""


CROP_FRAME = (48, 64, 3)  # h, w, channels of the seeded frame (seed 7)


def crop_cases():
    """Rects (x, y, w, h) inside, and hanging over every edge of, the 64 x 48 frame."""
    rng = np.random.default_rng(11)
    fixed = [(20, 14, 16, 16), (0, 0, 20, 20), (44, 28, 20, 20), (50, 2, 14, 10), (2, 30, 11, 17), (0, 0, 64, 48),
             (30, 20, 1, 1), (10, 10, 15, 9)]
    rand = [(int(x), int(y), int(w), int(h)) for x, y, w, h in
            zip(rng.integers(0, 50, 24), rng.integers(0, 36, 24), rng.integers(2, 30, 24), rng.integers(2, 30, 24))]
    return fixed + rand


def crop_frame():
    return np.random.default_rng(7).integers(0, 256, CROP_FRAME, dtype=np.uint8)


def reference_crops(ref_dir):
    src = open(os.path.join(ref_dir, "camera_face_demo.py")).read()
    fn = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "crop_face"][0]
    scale = None  # entity.py imports the networks: its 'face_crop_scale' entry is read from the source
    for node in ast.walk(ast.parse(open(os.path.join(ref_dir, "entity.py")).read())):
        if isinstance(node, ast.Dict):
            for k, v in zip(node.keys, node.values):
                if isinstance(k, ast.Constant) and k.value == "face_crop_scale":
                    scale = ast.literal_eval(v)
    space = {"np": np, "params": {"face_crop_scale": scale}}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "camera_face_demo.py", "exec"), space)
    frame, out = crop_frame(), []
    for rect in crop_cases():
        padded, left_top = space["crop_face"](frame, rect)
        out.append({"rect": list(rect), "left_top": [int(v) for v in left_top], "side": int(padded.shape[0]),
                    "sha1": hashlib.sha1(np.ascontiguousarray(padded).tobytes()).hexdigest()})
    return out


def main():
    os.makedirs(HERE, exist_ok=True)
    if "--reference" in sys.argv:
        with open(os.path.join(HERE, "crop_face_ref.json"), "w") as f:
            cases = reference_crops(sys.argv[sys.argv.index("--reference") + 1])
            f.write("{\"frame\": %s, \"frame_seed\": 7, \"cases\": [\n%s\n]}\n"
                    % (json.dumps(list(CROP_FRAME)), ",\n".join(json.dumps(c) for c in cases)))
        print("crop_face_ref.json")
    one = [TINY_STAGES[0]]
    files = {
        "tiny_cascade.xml": cascade_xml(6, 5, TINY_FEATURES, TINY_STAGES),
        "refuse_tilted.xml": cascade_xml(6, 5, TINY_FEATURES[:3], one, tilted=(1,)),
        "refuse_tree.xml": cascade_xml(6, 5, TINY_FEATURES[:3], one, nodes="1 -1 0 0.01 0 -1 1 0.02"),
        "refuse_lbp.xml": cascade_xml(6, 5, TINY_FEATURES[:3], one, feature_type="LBP"),
        "refuse_hog.xml": cascade_xml(6, 5, TINY_FEATURES[:3], one, feature_type="HOG"),
        "refuse_old_format.xml": OLD_FORMAT,
        "refuse_window.xml": cascade_xml(65, 5, TINY_FEATURES[:3], one),
        "refuse_rect_outside.xml": cascade_xml(6, 5, [TINY_FEATURES[0], TINY_FEATURES[1], [(0, 0, 6, 5, -1.0), (3, 0, 4, 5, 2.0)]], one),
    }
    for name, text in files.items():
        with open(os.path.join(HERE, name), "w") as f:
            f.write(text)
        print(name, len(text))


if __name__ == "__main__":
    main()
