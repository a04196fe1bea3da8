"""The index maps the kernels take their loop bounds, ownership tests and addresses from
(csrc/kernels/*_map.hpp), each walked on the CPU by a stand-alone program (csrc/kernels/test_*_map.cpp)
under AddressSanitizer + UndefinedBehaviorSanitizer.  ``WALKS`` names every program, the headers it is
rebuilt for and what it proves.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "csrc", "kernels")
FLAGS = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"]

# name -> (the headers test_<name>_map.cpp includes, what the walk proves)
WALKS = {
    "gbdt_hist": (
        ("gbdt_hist_map.hpp",),
        """The tile map of the GBDT histogram (csrc/kernels/gbdt_hist_map.hpp) on the CPU, under
        AddressSanitizer + UndefinedBehaviorSanitizer: csrc/kernels/test_gbdt_hist_map.cpp builds the clamped
        bounds and tile bases as the kernel does and walks every block and thread of the grid a launch builds,
        over benign and hostile segment tables (negative, non-monotone, past m, k = 0, m = 0), and checks that
        every owned (row slot, feature) is visited exactly once, by a block of the owning node, that every
        index is in range and every trip count inside its host-known bound.  No GPU."""),
    "gbdt_part": (
        ("gbdt_part_map.hpp", "gbdt_hist_map.hpp"),
        """The destination map of the GBDT row partition (csrc/kernels/gbdt_part_map.hpp) on the CPU, under
        AddressSanitizer + UndefinedBehaviorSanitizer: csrc/kernels/test_gbdt_part_map.cpp runs the count,
        offsets and scatter steps as plain loops over every tile, step and lane through the header, over benign
        and hostile segment tables, and checks that every defined output slot has exactly one writer inside
        ``[0, seg2[2k])`` and that every segment holds its node's rows in slot order.  No GPU."""),
    "moe_gemm": (
        ("moe_gemm_map.hpp",),
        """The tile map of the grouped expert GEMM (csrc/kernels/moe_gemm_map.hpp) on the CPU, under
        AddressSanitizer + UndefinedBehaviorSanitizer: csrc/kernels/test_moe_gemm_map.cpp walks every block id
        of every grid the launchers would build over benign and hostile segment tables and checks coverage
        exactly once, indices in range, trip counts inside their host-known bounds and the clamped segments.
        A kernel for the grouped GEMM takes every loop bound and row range from this header, so this is where
        its termination and addressing are tested.  No GPU."""),
    "moe_act": (
        ("moe_act_map.hpp",),
        """The row rule of the gated expert activation (csrc/kernels/moe_act_map.hpp) on the CPU, under
        AddressSanitizer + UndefinedBehaviorSanitizer: csrc/kernels/test_moe_act_map.cpp walks every wave and
        lane of the grids a launcher would build over benign and hostile segment tables and checks that a
        row is owned exactly where ``_table_segments`` says, that every (row, item) is visited once, that every
        index is in range and every trip count inside its host-known bound.  A kernel for the activation
        takes its ownership test and its row walk from this header, so this is where its termination and
        addressing are tested.  No GPU."""),
    "moe_prio": (
        ("moe_prio_map.hpp",),
        """The order of the per-expert top-S select (csrc/kernels/moe_prio_map.hpp) on the CPU, under
        AddressSanitizer + UndefinedBehaviorSanitizer: csrc/kernels/test_moe_prio_map.cpp checks the key
        against the float order for every special value, the word's tie rule, and runs the whole 8-pass radix
        select, with the histogram and digit step the kernel uses, against ``std::sort`` for every limit.
        The kernels take their order from this header only.  No GPU."""),
    "sparse_hash": (
        ("sparse_hash_map.hpp",),
        """The table of the canonical hash reduce-by-key (csrc/kernels/sparse_hash_map.hpp) on the CPU, under
        AddressSanitizer + UndefinedBehaviorSanitizer: csrc/kernels/test_sparse_hash_map.cpp runs the
        priority insertion with the header's step function, as the kernel runs it, from many shuffled row
        orders and with several simulated lanes taking single steps in turn, and compares the table with
        the plain insertion of the distinct keys in ascending order (t = 1024 slots, 1 to 512 rows,
        duplicates, keys with the top bit set, homes in the last 8 slots, one common home); the advance
        bound is never reached.  The kernels take the hash, the rule and the bounds from this header
        only.  No GPU."""),
}


def _build(name):
    """The walk's program under build/, rebuilt when any source it includes is newer."""
    out = os.path.join(ROOT, "build", f"test_{name}_map_asan")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    srcs = [os.path.join(KERNELS, f) for f in (f"test_{name}_map.cpp", "test_map_common.hpp") + WALKS[name][0]]
    if os.path.exists(out) and all(os.path.getmtime(out) > os.path.getmtime(s) for s in srcs):
        return out
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + FLAGS + [srcs[0], "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        probe = subprocess.run(["g++", "-x", "c++", "-", "-o", os.devnull] + FLAGS, input="int main(){}",
                               capture_output=True, text=True)
        if probe.returncode != 0:
            pytest.skip("sanitizer toolchain unavailable: " + probe.stderr[-500:])
        pytest.fail(f"the {name} map walk does not build:\n" + r.stderr[-3000:])
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
@pytest.mark.parametrize("name", sorted(WALKS))
def test_the_map_walk_passes_under_the_sanitizers(name):
    exe = _build(name)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.startswith("OK"), r.stdout[-1000:]
