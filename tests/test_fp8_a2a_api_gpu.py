"""alltoallArray with the fp8 operand through the public API (p processes sharing cuda:0).

The compressed calls are BIT-identical to the contract (tests/fp8_a2a_ref.py), return the exact
call's recvCounts and are counted as ``all_to_all_v.fp8.ipc`` alone; a row width off the 4-element
grid, an integer tensor, ``MP4X_FP8_TRANSPORT=rccl``, no operand or a send too large for the staging
buffers keep today's exact path, bit for bit, with no fp8 counter."""
import os

import pytest

torch = pytest.importorskip("torch")

from fp8_a2a_ref import CASES, exact_alltoall, expect_alltoall, inputs, same_bits  # noqa: E402
from spawn_ranks import run_spawn  # noqa: E402

pytestmark = pytest.mark.gpu

FP8, IPC = "all_to_all_v.fp8.ipc", "all_to_all_v.ipc"


def _api(comm):
    from mp4x import Operands
    r, p = comm.getRank(), comm.getSlaveNum()
    stats = comm.device.stats
    rows = []

    def call(send_cpu, counts, operand=None, recv=None, env=None):
        """One API call on a fresh device copy: (recv, recvCounts, the counters that moved)."""
        send = send_cpu.to("cuda")
        before = dict(stats)
        old = os.environ.get("MP4X_FP8_TRANSPORT")
        if env:
            os.environ["MP4X_FP8_TRANSPORT"] = env
        try:
            kw = {} if operand is None else dict(operand=operand)
            got, rc = comm.alltoallArray(send, counts, recv, **kw)
            torch.cuda.synchronize()
        finally:
            if env and old is None:
                del os.environ["MP4X_FP8_TRANSPORT"]
            elif env:
                os.environ["MP4X_FP8_TRANSPORT"] = old
        used = {k: c - before.get(k, 0) for k, c in stats.items() if c != before.get(k, 0)}
        return got, rc, used, same_bits(send.cpu(), send_cpu)

    for name in ("A", "B", "E"):
        dtype_name, w, mats = CASES[name]
        mat = mats[p]
        dt = getattr(torch, dtype_name)
        operand = (Operands.FLOAT_OPERAND if dt == torch.float32 else Operands.BF16_OPERAND)(codec="fp8")
        sends = inputs(mat, w, dt)
        want, want_counts, amb = expect_alltoall(sends, mat, w, r)
        got, rc, used, kept = call(sends[r], mat[r], operand)
        rows.append(dict(label=f"{name} fp8", equal=same_bits(got, want), counts=rc == want_counts, amb=amb,
                         fp8=used.get(FP8, 0), ipc=used.get(IPC, 0), kept=kept))
        # recvData supplied; on rank 1 a view at a 4-byte offset (f32) of a larger tensor
        n = want.numel()
        if r == 1 and dt == torch.float32:
            given = torch.zeros(n + 4, dtype=dt, device="cuda")[1:1 + n].view(want.shape)
            assert given.data_ptr() % 16 == 4
        else:
            given = torch.zeros(want.shape, dtype=dt, device="cuda")
        got, rc, used, kept = call(sends[r], mat[r], operand, recv=given)
        rows.append(dict(label=f"{name} fp8 into recvData", equal=same_bits(given, want) and got is given,
                         counts=rc == want_counts, amb=amb, fp8=used.get(FP8, 0), ipc=used.get(IPC, 0), kept=kept))

    # calls the codec does not apply to: the senders' rows exactly, no fp8 counter, and the counters
    # of the same call made without an operand
    _, w, mats = CASES["A"]
    mat = mats[p]
    f32 = Operands.FLOAT_OPERAND(codec="fp8")
    exact_cases = [
        ("w = 3 float32", inputs(mat, 3, torch.float32), f32, None),
        # the tensor's dtype decides, not the operand's
        ("int32", [(s * 1000).to(torch.int32) for s in inputs(mat, w, torch.float32)], f32, None),
        ("rccl transport", inputs(mat, w, torch.float32), f32, "rccl"),
        ("no operand", inputs(mat, w, torch.float32), None, None),
    ]
    for label, sends, operand, env in exact_cases:
        want = exact_alltoall(sends, mat, r)
        want_counts = [mat[k][r] for k in range(p)]
        _, _, plain_used, _ = call(sends[r], mat[r])
        got, rc, used, kept = call(sends[r], mat[r], operand, env=env)
        rows.append(dict(label=label, equal=same_bits(got, want), counts=rc == want_counts, amb=0,
                         fp8=used.get(FP8, 0), ipc=None, kept=kept, same_counters=used == plain_used,
                         used=used, plain_used=plain_used))
    return rows


def _too_large(comm):
    """A send whose codes exceed both staging buffers (shrunk by the environment): the fp8 form
    declines on every rank after the count exchange and the exact call runs with that matrix."""
    from mp4x import Operands
    r, p = comm.getRank(), comm.getSlaveNum()
    mat = [[20000, 13000], [5, 7]]                     # rank 0: 33000 rows of 64 f32 = 8250 quant blocks
    sends = inputs(mat, 64, torch.float32)
    stats = comm.device.stats
    from mp4x.parallel import sparse
    gathers, gather = [], sparse._count_matrix
    sparse._count_matrix = lambda *a: gathers.append(1) or gather(*a)
    try:
        got, rc = comm.alltoallArray(sends[r].to("cuda"), mat[r], operand=Operands.FLOAT_OPERAND(codec="fp8"))
    finally:
        sparse._count_matrix = gather
    torch.cuda.synchronize()
    return dict(equal=same_bits(got, exact_alltoall(sends, mat, r)), counts=rc == [mat[k][r] for k in range(p)],
                fp8=stats.get(FP8, 0), ipc=stats.get(IPC, 0), calls=stats.get("all_to_all_v", 0),
                gathers=len(gathers))


def test_a_send_too_large_for_the_staging_buffers_stays_exact():
    env = {"MP4X_IPC_BYTES": str(1 << 20), "MP4X_IPC_LARGE_BYTES": str(2 << 20)}    # 8065 blocks at most
    res = run_spawn(2, _too_large, env=env)
    assert sorted(res) == [0, 1]
    for r, row in res.items():
        assert row["equal"] and row["counts"], r
        assert (row["fp8"], row["ipc"], row["calls"]) == (0, 0, 1), (r, row)
        assert row["gathers"] == 1, (r, row)           # the declined form hands its matrix on


@pytest.mark.parametrize("p", [2, 3])
def test_fp8_operand_is_honoured_by_alltoall(p):
    res = run_spawn(p, _api)
    assert sorted(res) == list(range(p))
    for r, rows in res.items():
        assert len(rows) == 10
        for row in rows:
            what = (r, row["label"])
            assert row["amb"] == 0, what
            assert row["equal"], what
            assert row["counts"], what
            assert row["kept"], what
            if "fp8" in row["label"]:
                assert (row["fp8"], row["ipc"]) == (1, 0), (what, row["fp8"], row["ipc"])
            else:
                assert row["fp8"] == 0, what
                assert row["same_counters"], (what, row["used"], row["plain_used"])
