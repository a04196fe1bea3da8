"""The chunk plan and the step rule of the GBDT forest walk (csrc/kernels/gbdt_walk_map.hpp) on the CPU, under
AddressSanitizer + UndefinedBehaviorSanitizer: csrc/kernels/test_gbdt_walk_map.cpp, a stand-alone program,
runs a block of gbdt_predict.hip as plain loops through the header - the tile's bytes into an exactly sized
LDS image, the chunks, the walk of every row - over benign and hostile forests (a self-loop, a two-node
cycle, children outside the tree, a feature >= F, tree_off negative, non-monotone and past N, T = 0, a tree
of kChunkNodes + 1 nodes) and checks that every index is in range, every trip count inside its host-known
bound, that the chunks are disjoint, consecutive and cover every tree once and that the result equals a
direct evaluation of the definition.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "csrc", "kernels")
FLAGS = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_the_walk_map_passes_under_the_sanitizers():
    out = os.path.join(ROOT, "build", "test_gbdt_walk_map_asan")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + FLAGS + \
        [os.path.join(KERNELS, "test_gbdt_walk_map.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        probe = subprocess.run(["g++", "-x", "c++", "-", "-o", os.devnull] + FLAGS, input="int main(){}",
                               capture_output=True, text=True)
        if probe.returncode != 0:
            pytest.skip("sanitizer toolchain unavailable: " + probe.stderr[-500:])
        pytest.fail("the walk map test does not build:\n" + r.stderr[-3000:])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([out], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.startswith("OK"), r.stdout[-1000:]
