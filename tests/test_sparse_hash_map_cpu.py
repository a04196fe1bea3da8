"""The table of the canonical hash reduce-by-key (csrc/kernels/sparse_hash_map.hpp) on the CPU, under
AddressSanitizer + UndefinedBehaviorSanitizer: csrc/kernels/test_sparse_hash_map.cpp runs the
priority insertion with the header's step function, as the kernel runs it, from many shuffled row
orders and with several simulated lanes taking single steps in turn, and compares the table with
the plain insertion of the distinct keys in ascending order (t = 1024 slots, 1 to 512 rows,
duplicates, keys with the top bit set, homes in the last 8 slots, one common home); the advance
bound is never reached.  The kernels take the hash, the rule and the bounds from this header
only.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"]


def _build():
    out = os.path.join(ROOT, "build", "test_sparse_hash_map_asan")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    srcs = [os.path.join(ROOT, "csrc", "kernels", f) for f in ("test_sparse_hash_map.cpp", "sparse_hash_map.hpp")]
    if os.path.exists(out) and all(os.path.getmtime(out) > os.path.getmtime(s) for s in srcs):
        return out
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + FLAGS + [srcs[0], "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        probe = subprocess.run(["g++", "-x", "c++", "-", "-o", os.devnull] + FLAGS, input="int main(){}",
                               capture_output=True, text=True)
        if probe.returncode != 0:
            pytest.skip("sanitizer toolchain unavailable: " + probe.stderr[-500:])
        pytest.fail("the table test does not build:\n" + r.stderr[-3000:])
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_priority_insertion_builds_the_canonical_table_from_any_order():
    exe = _build()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.startswith("OK"), r.stdout[-1000:]
