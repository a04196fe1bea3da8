"""memAlloc: library-owned tensors mapped into every peer at ANY size (p processes on one GPU).

* a memAlloc tensor above 2 GiB (the size at which an IPC open of a caching-allocator
  allocation hangs, so ``registerBuffer`` refuses it) runs the zero-copy two-shot exactly,
  twice in a row (the second call reduces the first call's result in place);
* several physical chunks per tensor (``MP4X_VMM_CHUNK`` small) still give one contiguous
  tensor on every rank and one contiguous peer view;
* ZeRO-style reduce-scatter + all-gather of a bf16 memAlloc tensor take the zero-copy RS/AG
  kernels (no staging), exact;
* memFree releases it (a second memAlloc after the free works).
"""
import pytest

torch = pytest.importorskip("torch")

from spawn_ranks import run_spawn  # noqa: E402
from vmm_support import require_peer_vmm_import  # noqa: E402

pytestmark = pytest.mark.gpu


def _alloc_allreduce_fn(comm, n, reps):
    from mp4x import Operands, Operators
    r, p = comm.getRank(), comm.getSlaveNum()
    eng = comm.device
    t = comm.memAlloc(n, torch.float32)
    i = torch.arange(n, device="cuda", dtype=torch.int32) % 13
    t.copy_(i + r)
    exp = (i * p + p * (p - 1) // 2).float()
    before = dict(eng.stats)
    bad = []
    for k in range(reps):
        comm.allreduceArray(t, Operands.FLOAT_OPERAND(), Operators.Float.SUM, 0, n)
        torch.cuda.synchronize()
        bad.append(int((t != exp * (p ** k)).sum()))
    used = {k: v - before.get(k, 0) for k, v in eng.stats.items() if v != before.get(k, 0)}
    reg = eng._ipc_obj._find(t)[0]
    info = (t.numel(), t.is_contiguous(), len(reg.vmm) if reg else 0)
    comm.memFree(t)
    # the communicator still works, and a new allocation maps again (at the freed addresses)
    t2 = comm.memAlloc(1 << 20, torch.float32)
    i2 = torch.arange(1 << 20, device="cuda", dtype=torch.int32) % 11
    t2.copy_(i2 + r)
    comm.allreduceArray(t2, Operands.FLOAT_OPERAND(), Operators.Float.SUM, 0, 1 << 20)
    torch.cuda.synchronize()
    exp2 = (i2 * p + p * (p - 1) // 2).float()
    wrong = (t2 != exp2).nonzero().view(-1)
    ok2 = (int(wrong.numel()), [(int(j), float(t2[j]), float(exp2[j])) for j in wrong[:4].tolist()])
    ptr2 = t2.data_ptr()
    comm.memFree(t2)
    # same size again: exact (the pooled allocation itself under MP4X_VMM_POLICY=pool)
    t3 = comm.memAlloc(1 << 20, torch.float32)
    t3.copy_(i2 + r)
    comm.allreduceArray(t3, Operands.FLOAT_OPERAND(), Operators.Float.SUM, 0, 1 << 20)
    torch.cuda.synchronize()
    from mp4x.parallel import ipc as ipc_mod
    # under the pool policy the same allocation comes back; otherwise any address will do
    ok3 = (t3.data_ptr() == ptr2 or ipc_mod.VMM_POLICY != "pool", int((t3 != exp2).sum()))
    comm.memFree(t3)
    return bad, used, info, ok2 + ok3


def test_memalloc_above_2gib_zero_copy_exact():
    require_peer_vmm_import()
    n = (2 << 30) // 4 + (1 << 20)            # 2 GiB + 4 MiB of float32
    out = run_spawn(2, _alloc_allreduce_fn, args=(n, 2), timeout=300)
    for r, (bad, used, info, ok2) in out.items():
        assert bad == [0, 0], (r, bad)
        assert used.get("allreduce.ipc2z", 0) == 2, used
        assert info[0] == n and info[1], info
        assert ok2[0] == 0 and ok2[2] and ok2[3] == 0, (r, ok2)


def test_memalloc_many_chunks():
    require_peer_vmm_import()
    n = (40 << 20) // 4 + 16                    # 40 MiB + 64 B over 8 MiB chunks: 6 chunks
    out = run_spawn(3, _alloc_allreduce_fn, args=(n, 2), env={"MP4X_VMM_CHUNK": str(8 << 20)})
    for r, (bad, used, info, ok2) in out.items():
        assert bad == [0, 0], (r, bad)
        assert used.get("allreduce.ipc2z", 0) == 2, used
        assert info[2] >= 2 + 2 * 2, info       # own + scratch + two peers' tensor + scratch
        assert ok2[0] == 0 and ok2[2] and ok2[3] == 0, (r, ok2)


def _zero_fn(comm, n):
    from mp4x import Operands, Operators
    from mp4x.utils.commutils import CommUtils
    r, p = comm.getRank(), comm.getSlaveNum()
    eng = comm.device
    t = comm.memAlloc(n, torch.bfloat16)
    i = torch.arange(n, device="cuda", dtype=torch.int32) % 7
    t.copy_(i + r)
    counts = [(n // p) // 8 * 8] * p              # whole 16-byte vectors per segment
    counts[-1] += n - sum(counts)
    B = Operands.BF16_OPERAND()
    before = dict(eng.stats)
    comm.reduceScatterArray(t, B, Operators.BFloat16.SUM, 0, counts)
    froms, tos = CommUtils.getFromsFromCount(0, counts, p), CommUtils.getTosFromCount(0, counts, p)
    exp = (i * p + p * (p - 1) // 2).to(torch.bfloat16)
    bad_rs = int((t[froms[r]:tos[r]] != exp[froms[r]:tos[r]]).sum())
    comm.allgatherArray(t, B, froms, tos)
    torch.cuda.synchronize()
    bad_ag = int((t != exp).sum())
    used = {k: v - before.get(k, 0) for k, v in eng.stats.items() if v != before.get(k, 0)}
    comm.memFree(t)
    return bad_rs, bad_ag, used


def test_memalloc_zero_rs_ag_bf16():
    n = (96 << 20) // 2                           # 96 MiB of bf16, above the staging buffer
    out = run_spawn(4, _zero_fn, args=(n,))
    for r, (bad_rs, bad_ag, used) in out.items():
        assert bad_rs == 0 and bad_ag == 0, (r, bad_rs, bad_ag, used)
        assert used.get("reduce_scatter.ipc_zc") == 1 and used.get("allgather.ipc_zc") == 1, used


def _fp8_whole_fn(comm, n):
    from mp4x import Operands, Operators
    r, p = comm.getRank(), comm.getSlaveNum()
    eng = comm.device

    def gen(j):
        return torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7 + j))
    x = gen(r)
    comm.allreduceArray(x, Operands.FLOAT_OPERAND(codec="fp8"), Operators.Float.SUM, 0, n)
    torch.cuda.synchronize()
    idx = torch.arange(0, n, 997, device="cuda")          # strided sample vs the fp64 sum
    ref = sum(gen(j)[idx].double() for j in range(p))
    mag = sum(gen(j)[idx].double().abs() for j in range(p))
    err = (x[idx].double() - ref).abs()
    nbad = int((err > (mag + ref.abs()) / 8 + 1e-3).sum())
    big = eng._ipc_fp8_big
    return nbad, dict(eng.stats), (big is not None and big._vmm_data, big.nbytes if big else 0)


def test_fp8_whole_tensor_staging_built_from_vmm():
    require_peer_vmm_import()
    # the open limit lowered to 64 MiB so a ~85 MB quantised tensor needs the VMM-built staging
    # buffer (the path BASELINE config 5, 8 GB of f32 -> 2 GB of e4m3, takes at the real limit)
    n = 80 << 20
    out = run_spawn(2, _fp8_whole_fn, args=(n,), env={"MP4X_IPC_OPEN_MAX": str(64 << 20)})
    for r, (nbad, stats, (is_vmm, nb)) in out.items():
        assert nbad == 0, (r, nbad)
        assert stats.get("allreduce.fp8.ipc", 0) == 1, stats
        assert is_vmm and nb >= n * 260 // 256, (is_vmm, nb)


def _standin_fn(comm, n):
    from mp4x import Operands, Operators
    r, p = comm.getRank(), comm.getSlaveNum()
    eng = comm.device
    t = comm.memAlloc(n, torch.float32)
    reg = eng._ipc_obj._find(t)[0]
    kind = (reg is not None, bool(reg.vmm) if reg is not None else None)
    i = torch.arange(n, device="cuda", dtype=torch.int32) % 13
    t.copy_(i + r)
    before = dict(eng.stats)
    comm.allreduceArray(t, Operands.FLOAT_OPERAND(), Operators.Float.SUM, 0, n)
    torch.cuda.synchronize()
    bad = int((t != (i * p + p * (p - 1) // 2).float()).sum())
    used = {k: v - before.get(k, 0) for k, v in eng.stats.items() if v != before.get(k, 0)}
    comm.memFree(t)
    return kind, bad, used, eng._zc, eng._zc_vmm, eng._ipc_obj._find(t)[0] is None


def test_memalloc_falls_back_to_registered_plain_tensors_when_only_its_self_test_fails():
    """The memAlloc (VMM) self-test fails on one rank (injected): every rank keeps the zero-copy
    forms for registered tensors, memAlloc hands out a registered plain tensor, the allreduce on
    it is the zero-copy two-shot and exact, memFree deregisters it."""
    n = (8 << 20) // 4
    out = run_spawn(2, _standin_fn, args=(n,), env={"MP4X_IPC_SELFTEST_INJECT_MEMALLOC": "1"})
    for r, (kind, bad, used, zc, zc_vmm, gone) in out.items():
        assert zc and not zc_vmm, (r, zc, zc_vmm)
        assert kind == (True, False), kind                  # registered, not VMM-built
        assert bad == 0 and used.get("allreduce.ipc2z", 0) + used.get("allreduce.ipc2w", 0) == 1, used
        assert gone
