"""csrc/jpeg_host.hpp over hostile input under AddressSanitizer and UBSan: tests/jpeg_host_main.cpp
(a stand-alone program, no GPU, no library; the environment is passed on as it is) runs the header
parse and the entropy decode on every prefix of two small fixtures and on the files with every byte replaced by 0x00, 0xFF
and its complement.  Every call must return a status: no crash, no sanitizer report, no leak."""
import os
import shutil
import subprocess

import pytest

import jpeg_cases as cases
from conftest import PKG_NAME, REPO

FIXTURES = ("16x16_420_q20.jpg", "37x45_420_q75_restart_blocks2.jpg")
STRIDE = 1  # every byte position is mutated


@pytest.mark.skipif(not shutil.which("g++"), reason="no g++")
def test_hostile_input_under_sanitizers(tmp_path):
    exe = str(tmp_path / "jpeg_host_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-pthread",
                    # the runtimes are linked statically: the program starts whatever the environment preloads
                    "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(REPO, PKG_NAME, "csrc"), os.path.join(REPO, "tests", "jpeg_host_main.cpp"),
                    "-o", exe], check=True, timeout=300)
    paths = [os.path.join(cases.DIR, n) for n in FIXTURES]
    assert all(500 <= os.path.getsize(p) <= 1000 for p in paths)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe, str(STRIDE)] + paths, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "jpeg host ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-6000:])
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-6000:]
    calls = sum(os.path.getsize(q) * 4 + 1 for q in paths)
    assert p.stdout.startswith("jpeg host ok: %d calls" % calls), p.stdout
