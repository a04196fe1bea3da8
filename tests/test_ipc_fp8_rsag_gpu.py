"""The halves of the fp8 two-shot as collectives of their own (csrc/runtime/ipc.hip k_ipc_fp8_rs /
k_ipc_fp8_ag; IpcAllreduce.reduce_scatter_fp8 / allgather_fp8), p processes sharing ONE GPU, a
64 KiB staging buffer so the larger cases run in several pieces.  The results must be BIT-identical
to the contract computed with the CPU reference of the K6 codec (tests/fp8_rsag_ref.py): one
quantisation, an f32 sum in rank order, one rounding; nothing outside a rank's segment (reduce-
scatter) or outside the range (all-gather) is written."""
import hashlib

import pytest

torch = pytest.importorskip("torch")

from fp8_rsag_ref import CASES, bounds, expect_allgather, expect_reduce_scatter, inputs, same_bits  # noqa: E402
from spawn_ranks import run_spawn  # noqa: E402

pytestmark = pytest.mark.gpu


def _digest(t):
    return hashlib.sha1(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def _one(ipc, half, x, frm, counts, r, offset_rank=None):
    """Run one half on this rank's copy of ``x`` (at a 4-byte offset on ``offset_rank``): the
    tensor afterwards, what the call returned, the error word."""
    n = x.numel()
    if offset_rank == r:
        assert x.element_size() == 4
        buf = torch.empty(n + 4, dtype=x.dtype, device="cuda")
        y = buf[1:1 + n]
        assert y.data_ptr() % 16 == 4
    else:
        y = torch.empty(n, dtype=x.dtype, device="cuda")
    y.copy_(x)
    froms, tos = bounds(frm, counts)
    ok = (ipc.reduce_scatter_fp8 if half == "rs" else ipc.allgather_fp8)(y, froms, tos)
    torch.cuda.synchronize()
    return y.cpu(), ok, ipc.error_word()


def _worker(comm):
    from mp4x.parallel.ipc import IpcAllreduce
    r, p = comm.getRank(), comm.getSlaveNum()
    ipc = IpcAllreduce(comm, nbytes=64 << 10)
    out = []
    runs = [(name, None) for name in CASES] + [("A", 1)]      # case A again, rank 1's tensor offset by 4 bytes
    for name, offset_rank in runs:
        dtype_name, n, frm, counts = CASES[name]
        counts = counts[p]
        xs = inputs(n, getattr(torch, dtype_name), p)
        froms, tos = bounds(frm, counts)
        for half, expect in (("rs", expect_reduce_scatter), ("ag", expect_allgather)):
            want, amb = expect(xs, r, frm, counts)
            got, ok, ew = _one(ipc, half, xs[r], frm, counts, r, offset_rank)
            # untouched: everything but the own segment (rs) / but the range (ag)
            keep = torch.ones(n, dtype=torch.bool)
            if half == "rs":
                keep[froms[r]:tos[r]] = False
            else:
                keep[froms[0]:tos[-1]] = False
            diff = (got.view(torch.uint8).view(n, -1) != want.view(torch.uint8).view(n, -1)).any(dim=1).nonzero().view(-1)
            out.append(dict(case=name, half=half, offset=offset_rank, ok=bool(ok), amb=amb, ew=ew,
                            equal=same_bits(got, want), untouched=same_bits(got[keep], xs[r][keep]),
                            ndiff=int(diff.numel()), first=int(diff[0]) if diff.numel() else -1,
                            range_digest=_digest(got[froms[0]:tos[-1]])))
    comm.barrier()
    ipc.close()
    return out


@pytest.mark.parametrize("p", [2, 3])
def test_fp8_halves_match_the_contract_bit_for_bit(p):
    res = run_spawn(p, _worker)
    assert sorted(res) == list(range(p))
    nrun = len(res[0])
    assert nrun == 2 * (len(CASES) + 1)
    for i in range(nrun):
        rows = [res[r][i] for r in range(p)]
        for r, row in enumerate(rows):
            what = (row["case"], row["half"], row["offset"], r)
            assert row["amb"] == 0, what          # a condition on the inputs: change a seed, never the comparison
            assert row["ok"], what
            assert row["ew"] == 0, what
            assert row["equal"], (what, row["ndiff"], row["first"])
            assert row["untouched"], what
        if rows[0]["half"] == "ag":               # every rank holds the same bytes, own segment included
            assert len({row["range_digest"] for row in rows}) == 1, rows[0]["case"]
