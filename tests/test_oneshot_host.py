"""csrc/oneshot.hip's failure path, executed (no GPU: every HIP call fails with hipErrorNoDevice):
tests/oneshot_fail_main.cpp and oneshot.hip are compiled into one program with the host code under
AddressSanitizer, and the program drives a job through its whole step list after its first
allocation failed.  It must keep the first error, hand out no buffer, touch no memory it does not
own and leak nothing (ASan's leak check runs when it exits)."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG_NAME, REPO

CSRC = os.path.join(REPO, PKG_NAME, "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")
def test_job_failure_path_under_asan(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the HIP calls would succeed")
    exe = str(tmp_path / "oneshot_fail")
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    objs = []
    for src in (os.path.join(REPO, "tests", "oneshot_fail_main.cpp"), os.path.join(CSRC, "oneshot.hip")):
        objs.append(str(tmp_path / (os.path.basename(src) + ".o")))
        # the host code alone is instrumented, as in csrc/Makefile's asan objects
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall",
                        "-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fno-omit-frame-pointer",
                        "-I", os.path.join(REPO, "include"), "-I", CSRC, "-x", "hip", "-c", src, "-o", objs[-1]],
                       check=True, timeout=300)
    subprocess.run([hipcc, "-Xarch_host", "-fsanitize=address"] + objs + ["-o", exe], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", HIP_VISIBLE_DEVICES="",
               ROCR_VISIBLE_DEVICES="")
    p = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "oneshot ok" in p.stdout, (p.returncode, p.stdout[-3000:], p.stderr[-6000:])
    assert "Sanitizer" not in p.stderr, p.stderr[-6000:]
