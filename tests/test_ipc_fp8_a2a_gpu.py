"""The fp8 ragged all-to-all (csrc/runtime/ipc.hip k_ipc_fp8_a2a; IpcAllreduce.alltoall_fp8), p
processes sharing ONE GPU, a 64 KiB staging buffer.  The received rows must be BIT-identical to the
contract computed with the CPU reference of the K6 codec (tests/fp8_a2a_ref.py): each sender's whole
buffer quantised once on one block grid, decoded with fma(code, scale, +0), one rounding; nothing
outside the receive tensor is written, the send tensor keeps its bits; a send that does not fit the
buffer is declined on every rank with the epoch unmoved."""
import pytest

torch = pytest.importorskip("torch")

from fp8_a2a_ref import CASES, TOO_LARGE, expect_alltoall, inputs, same_bits  # noqa: E402
from spawn_ranks import run_spawn  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = 64


def _one(ipc, send_cpu, mat, w, r, offset_rank=None):
    """One call on this rank's device copy of ``send_cpu`` (at a 4-byte offset on ``offset_rank``),
    the receive tensor in the middle of a canary-filled buffer."""
    n = send_cpu.numel()
    if offset_rank == r:
        assert send_cpu.element_size() == 4
        buf = torch.empty(n + 4, dtype=send_cpu.dtype, device="cuda")
        send = buf[1:1 + n].view(-1, w)
        assert send.data_ptr() % 16 == 4
    else:
        send = torch.empty(send_cpu.shape, dtype=send_cpu.dtype, device="cuda")
    send.copy_(send_cpu)
    rows = sum(mat[k][r] for k in range(len(mat)))
    guard = torch.full((2 * CANARY + rows * w,), 7.0, dtype=send_cpu.dtype, device="cuda")
    recv = guard[CANARY:CANARY + rows * w].view(rows, w)
    before = ipc.epoch
    ok = ipc.alltoall_fp8(send, mat, recv)
    torch.cuda.synchronize()
    g = guard.cpu()
    return dict(ok=bool(ok), ew=ipc.error_word(), recv=g[CANARY:CANARY + rows * w].view(rows, w),
                canary=bool((g[:CANARY] == 7).all() and (g[CANARY + rows * w:] == 7).all()),
                send_kept=same_bits(send.cpu(), send_cpu), epoch_moved=ipc.epoch != before)


def _worker(comm):
    from mp4x.parallel.ipc import IpcAllreduce
    r, p = comm.getRank(), comm.getSlaveNum()
    ipc = IpcAllreduce(comm, nbytes=64 << 10)
    out = []
    # every case, case A again with rank 1's send tensor offset by 4 bytes, the send that does not
    # fit, and case A after it (the epochs stayed in step)
    runs = [(name, CASES[name], None) for name in CASES] + [("A", CASES["A"], 1), ("big", TOO_LARGE, None),
                                                            ("A", CASES["A"], None)]
    for name, (dtype_name, w, mats), offset_rank in runs:
        mat = mats[p]
        sends = inputs(mat, w, getattr(torch, dtype_name))
        got = _one(ipc, sends[r], mat, w, r, offset_rank)
        row = dict(case=name, offset=offset_rank, ok=got["ok"], ew=got["ew"], canary=got["canary"],
                   send_kept=got["send_kept"], epoch_moved=got["epoch_moved"])
        if name == "big":
            row["untouched"] = bool((got["recv"] == 7).all())
        else:
            want, _, amb = expect_alltoall(sends, mat, w, r)
            diff = (got["recv"] != want).any(dim=1).nonzero().view(-1) if want.numel() else torch.empty(0)
            row.update(amb=amb, equal=same_bits(got["recv"], want), ndiff=int(diff.numel()),
                       first=int(diff[0]) if diff.numel() else -1)
        out.append(row)
    # the shared-GPU grid cap of family "fp8a2a", from both of its sources
    import ctypes
    from mp4x.operators import DType
    from mp4x.parallel import occupancy
    api = ctypes.c_int(0)
    rc = ipc.lib.mp4x_ipc_occupancy_misc(IpcAllreduce._OCC_FAMILY["fp8a2a"], int(DType.F32), p, ctypes.byref(api))
    cap = dict(shared=bool(ipc.shared_gpu), cap=ipc.grid_cap("fp8a2a", torch.float32), rc=rc, api=api.value,
               table=occupancy.table_bpc("fp8a2a", int(DType.F32), "F32", 0, p))
    comm.barrier()
    ipc.close()
    return out, cap


@pytest.mark.parametrize("p", [2, 3])
def test_fp8_alltoall_matches_the_contract_bit_for_bit(p):
    res = run_spawn(p, _worker)
    assert sorted(res) == list(range(p))
    assert len(res[0][0]) == len(CASES) + 3
    assert len({res[r][1]["cap"] for r in range(p)}) == 1          # every rank launches under the same cap
    for r in range(p):
        cap = res[r][1]
        assert cap["shared"] and cap["rc"] == 0 and cap["api"] >= 1 and cap["table"] and cap["table"] >= 1, cap
        assert 1 <= cap["cap"] <= 256, cap
        for row in res[r][0]:
            what = (row["case"], row["offset"], r)
            assert row["ew"] == 0, what
            assert row["canary"], what
            assert row["send_kept"], what
            if row["case"] == "big":                  # declined: nothing done, the epoch unmoved
                assert not row["ok"], what
                assert row["untouched"], what
                assert not row["epoch_moved"], what
                continue
            assert row["amb"] == 0, what              # a condition on the inputs: change a seed, never the comparison
            assert row["ok"], what
            assert row["equal"], (what, row["ndiff"], row["first"])
            assert row["epoch_moved"], what
