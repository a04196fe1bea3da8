"""memFree policies side by side ("hipMemRelease of VMM then re-import reading
zeros").  Each policy (``MP4X_VMM_POLICY``, parallel/ipc.py) runs, in 2 ranks:

* the memAlloc self-test — memAlloc, the zero-copy two-shot (pull and push, each twice), memFree,
  then a SECOND memAlloc of another size through the same kernels — twice over;
* CYCLES memAlloc / allreduce / memFree cycles of distinct sizes, exact, with the device memory in
  use sampled after every cycle (``torch.cuda.mem_get_info``: both ranks' memory, shared GPU).

Every row is written to the progress log (``MP4X_TEST_PROGRESS``) as evidence.  Asserted: the
DEFAULT policy is exact and bounded; ``pool`` and ``fresh_va`` are exact (their growth is the sum
of the distinct sizes: pool by design, fresh_va because this runtime never gives a released
exported chunk back).  The other rows are the lifetime study — the policies that free a VA
range, which this runtime answers with wrong reads — and are recorded, not asserted.
"""
import json
import os

import pytest

torch = pytest.importorskip("torch")

from spawn_ranks import run_spawn  # noqa: E402
from vmm_support import require_peer_vmm_import  # noqa: E402

pytestmark = pytest.mark.gpu

CYCLES = 12
BOUND_MB = 256


def _used():
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info()
    return total - free


def _policy_fn(comm):
    from mp4x import Operands, Operators
    from mp4x.parallel import ipc as ipc_mod
    from mp4x.parallel import vmm
    r, p = comm.getRank(), comm.getSlaveNum()
    inst = comm.device.ipc()
    assert inst is not None
    selftest = [inst.selftest_memalloc(1 << 18) for _ in range(2)]
    comm.barrier()
    torch.cuda.empty_cache()
    used0 = _used()
    bad, growth, ptrs = 0, [], []
    for k in range(CYCLES):
        n = (8 << 20) // 4 + k * (512 << 10)             # 8 MiB + k * 2 MiB
        t = comm.memAlloc(n, torch.float32)
        ptrs.append(t.data_ptr())
        i = torch.arange(n, device="cuda", dtype=torch.int32) % 13
        t.copy_((i + r + k).float())
        comm.allreduceArray(t, Operands.FLOAT_OPERAND(), Operators.Float.SUM, 0, n)
        torch.cuda.synchronize()
        bad += int((t != (i * p + p * (p - 1) // 2 + k * p).float()).sum())
        del i
        comm.memFree(t)
        del t
        comm.barrier()
        torch.cuda.empty_cache()          # the caching allocator's temporaries are not memAlloc's
        growth.append(round((_used() - used0) / 2**20, 1))
    return {"policy": ipc_mod.VMM_POLICY, "selftest_bad": selftest, "cycles_bad": bad,
            "growth_mb": growth, "recycled_own_va": len(ptrs) - len(set(ptrs)),
            "quarantined_va_mb": vmm.quarantined_bytes() >> 20, "stats": {
                k: v for k, v in comm.device.stats.items() if k.startswith("allreduce.")}}


def _note(row):
    path = os.environ.get("MP4X_TEST_PROGRESS")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"vmm_policy": row}) + "\n")


@pytest.mark.parametrize("policy", ["chunks", "fresh_va", "hint", "keep_owner_va", "keep_import_va", "ordered", "pool"])
def test_memfree_policy(policy):
    from mp4x.parallel import ipc as ipc_mod
    if policy in (ipc_mod.VMM_POLICY, "pool", "fresh_va"):
        require_peer_vmm_import()           # the asserted rows are about peer-mapped memory
    env = {"MP4X_VMM_POLICY": policy, "MP4X_IPC_SELFTEST": "0"}
    out = run_spawn(2, _policy_fn, env=env, timeout=200)
    _note({"policy": policy, "ranks": out})
    assert all(v["policy"] == policy for v in out.values()), out
    if policy in (ipc_mod.VMM_POLICY, "pool", "fresh_va"):
        for r, v in out.items():
            assert v["selftest_bad"] == [0, 0] and v["cycles_bad"] == 0, (policy, r, v)
    if policy == ipc_mod.VMM_POLICY:
        for r, v in out.items():
            assert max(v["growth_mb"]) <= BOUND_MB, (policy, r, v["growth_mb"])
