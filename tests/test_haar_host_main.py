"""csrc/haar_host.hpp as a stand-alone program (tests/haar_host_main.cpp: no GPU, no library): the
classes it makes of a few hundred seeded rectangles and the scale lists of a few frames equal
haar.py's statement, built plainly and under AddressSanitizer + UBSan (its own executable, the
runtimes linked statically, nothing preloaded)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import haar_cases as cases
from conftest import PKG_NAME, REPO

H = cases.haar()
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan",
            "-static-libubsan"]


@pytest.mark.skipif(not shutil.which("g++"), reason="no g++")
@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g"] + SANITIZE], ids=["plain", "sanitized"])
def test_grouping_and_scales_equal_the_statement(tmp_path, flags):
    exe = str(tmp_path / "haar_host_main")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags +
                   ["-I", os.path.join(REPO, PKG_NAME, "csrc"), os.path.join(REPO, "tests", "haar_host_main.cpp"), "-o", exe],
                   check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe, "5", "300"], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.endswith("haar host ok\n"), (p.returncode, p.stdout[-2000:], p.stderr[-6000:])
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-6000:]
    lines = [l.split() for l in p.stdout.splitlines()]
    rects = np.array([[int(v) for v in l[1:]] for l in lines if l[0] == "in"], np.int32)
    assert rects.shape == (300, 4)
    groups = 0
    for min_neighbors in (0, 1, 3, 6):
        got = np.array([[int(v) for v in l[2:]] for l in lines if l[0] == "group" and int(l[1]) == min_neighbors],
                       np.int32).reshape(-1, 5)
        r, n = H.group_rectangles_np(rects, min_neighbors)
        assert np.array_equal(got[:, :4], r) and np.array_equal(got[:, 4], n), min_neighbors
        groups += len(r) if min_neighbors else 0
    assert groups >= 6  # classes were formed, kept and (at 6) dropped
    seen = 0
    for l in lines:
        if l[0] != "scales":
            continue
        h, w, factor, count = int(l[1]), int(l[2]), float(l[3]), int(l[4])
        try:
            want = H.scales(h, w, (20, 20), factor)
        except ValueError:
            assert count == -1, l[:5]  # more than 64 scales
            seen += 1
            continue
        assert count == len(want), l[:5]
        for item, (sc, lw, lh) in zip(l[5:], want):
            a, b, c = item.split(":")
            assert np.float32(float(a)) == sc and (int(b), int(c)) == (lw, lh), (l[:5], item)
    assert seen >= 2
