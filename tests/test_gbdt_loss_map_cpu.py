"""The GBDT loss rules (csrc/kernels/gbdt_loss_map.hpp) on the CPU, under AddressSanitizer +
UndefinedBehaviorSanitizer: csrc/kernels/test_gbdt_loss_map.cpp, a stand-alone program, runs the header the
kernels compile over the hostile margins and a seeded spread and checks ``exp_neg`` against ``expl`` within 4 ulp,
every intermediate integer and shift inside its range and the special rows by value.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "csrc", "kernels")
FLAGS = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_the_loss_map_passes_under_the_sanitizers():
    out = os.path.join(ROOT, "build", "test_gbdt_loss_map_asan")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + FLAGS + \
        [os.path.join(KERNELS, "test_gbdt_loss_map.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        probe = subprocess.run(["g++", "-x", "c++", "-", "-o", os.devnull] + FLAGS, input="int main(){}",
                               capture_output=True, text=True)
        if probe.returncode != 0:
            pytest.skip("sanitizer toolchain unavailable: " + probe.stderr[-500:])
        pytest.fail("the loss map test does not build:\n" + r.stderr[-3000:])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([out], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.startswith("OK"), r.stdout[-1000:]
