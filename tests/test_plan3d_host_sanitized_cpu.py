"""The 3D pass geometry (csrc/runtime/plan3d.cpp) under AddressSanitizer + UBSan:
a stand-alone program (tests/native/plan3d_selftest.cpp, its own ``main``) walks
the hand cases of tests/test_plan3d_cpu.py and a sweep of small tiles. Built
with g++ -fsanitize=address,undefined and run as a program: nothing is loaded
into Python and nothing is preloaded."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_plan3d_selftest_asan_ubsan(tmp_path):
    exe = tmp_path / "plan3d_selftest"
    srcs = [os.path.join(ROOT, "tests", "native", "plan3d_selftest.cpp"),
            os.path.join(ROOT, "csrc", "runtime", "plan3d.cpp"),
            os.path.join(ROOT, "csrc", "kernels", "kernel_select.cpp"),
            os.path.join(ROOT, "csrc", "runtime", "errors.cpp")]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "csrc", "include"), *srcs, "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ,  # as tests/test_native_host_asan.py runs its program
               ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "plan3d selftest OK" in r.stdout
