"""The order of the per-expert top-S select (csrc/kernels/moe_prio_map.hpp) on the CPU, under
AddressSanitizer + UndefinedBehaviorSanitizer: csrc/kernels/test_moe_prio_map.cpp checks the key
against the float order for every special value, the word's tie rule, and runs the whole 8-pass radix
select, with the histogram and digit step the kernel uses, against ``std::sort`` for every limit.
The kernels take their order from this header only.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"]


def _build():
    out = os.path.join(ROOT, "build", "test_moe_prio_map_asan")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    srcs = [os.path.join(ROOT, "csrc", "kernels", f) for f in ("test_moe_prio_map.cpp", "moe_prio_map.hpp")]
    if os.path.exists(out) and all(os.path.getmtime(out) > os.path.getmtime(s) for s in srcs):
        return out
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + FLAGS + [srcs[0], "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        probe = subprocess.run(["g++", "-x", "c++", "-", "-o", os.devnull] + FLAGS, input="int main(){}",
                               capture_output=True, text=True)
        if probe.returncode != 0:
            pytest.skip("sanitizer toolchain unavailable: " + probe.stderr[-500:])
        pytest.fail("the select test does not build:\n" + r.stderr[-3000:])
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_the_radix_select_finds_what_std_sort_finds():
    exe = _build()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.startswith("OK"), r.stdout[-1000:]
