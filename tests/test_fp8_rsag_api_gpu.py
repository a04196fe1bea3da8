"""reduceScatterArray / allgatherArray with the fp8 operand through the public API (p = 2 processes
sharing cuda:0), and ZeroOptimizer(grad_codec="fp8") on top of it.

The compressed calls are BIT-identical to the contract (tests/fp8_rsag_ref.py) and counted as
``reduce_scatter.fp8.ipc`` / ``allgather.fp8.ipc``; another operator, offsets off the 16-byte grid
or ``MP4X_FP8_TRANSPORT=rccl`` keep today's exact path, bit for bit, and move no fp8 counter."""
import os

import pytest

torch = pytest.importorskip("torch")

from fp8_rsag_ref import CASES, bounds, expect_allgather, expect_reduce_scatter, inputs, same_bits  # noqa: E402
from spawn_ranks import run_spawn  # noqa: E402

pytestmark = pytest.mark.gpu

RS, AG = "reduce_scatter.fp8.ipc", "allgather.fp8.ipc"


def _api(comm):
    from mp4x import Operands, Operators
    r, p = comm.getRank(), comm.getSlaveNum()
    stats = comm.device.stats
    rows = []

    def count():
        return stats.get(RS, 0), stats.get(AG, 0)

    def call(kind, x, operand, operator, frm, counts, env=None):
        """One API call on a fresh device copy of ``x``: (result on the CPU, counter deltas)."""
        y = x.to("cuda")
        before = count()
        old = os.environ.get("MP4X_FP8_TRANSPORT")
        if env:
            os.environ["MP4X_FP8_TRANSPORT"] = env
        try:
            if kind == "rs":
                comm.reduceScatterArray(y, operand, operator, frm, list(counts))
            else:
                froms, tos = bounds(frm, counts)
                comm.allgatherArray(y, operand, froms, tos)
            torch.cuda.synchronize()
        finally:
            if env and old is None:
                del os.environ["MP4X_FP8_TRANSPORT"]
            elif env:
                os.environ["MP4X_FP8_TRANSPORT"] = old
        after = count()
        return y.cpu(), (after[0] - before[0], after[1] - before[1])

    for name in ("A", "D"):
        dtype_name, n, frm, counts = CASES[name]
        counts = counts[p]
        dt = getattr(torch, dtype_name)
        make = Operands.FLOAT_OPERAND if dt == torch.float32 else Operands.BF16_OPERAND
        operand, plain = make(codec="fp8"), make()
        xs = inputs(n, dt, p)
        x = xs[r]

        def exact_rs(cnts, fold):
            froms, tos = bounds(frm, cnts)
            out = x.clone()
            out[froms[r]:tos[r]] = fold(xs[0][froms[r]:tos[r]], xs[1][froms[r]:tos[r]])
            return out

        def exact_ag(cnts):
            froms, tos = bounds(frm, cnts)
            out = x.clone()
            for k in range(p):
                out[froms[k]:tos[k]] = xs[k][froms[k]:tos[k]]
            return out

        odd = [258, 510]                                   # offsets that are no 16-byte multiples
        want_rs, amb_rs = expect_reduce_scatter(xs, r, frm, counts)
        want_ag, amb_ag = expect_allgather(xs, r, frm, counts)
        checks = [
            # (label, kind, operator, counts, "rccl" = that transport / "plain" = no codec, expected
            #  result, expected counter deltas)
            ("fp8", "rs", Operators.Float.SUM, counts, None, want_rs, (1, 0)),
            ("fp8 again", "rs", Operators.Float.SUM, counts, None, want_rs, (1, 0)),
            ("max", "rs", Operators.Float.MAX, counts, None, exact_rs(counts, torch.maximum), (0, 0)),
            ("odd offsets", "rs", Operators.Float.SUM, odd, None, exact_rs(odd, torch.add), (0, 0)),
            ("rccl transport", "rs", Operators.Float.SUM, counts, "rccl", exact_rs(counts, torch.add), (0, 0)),
            # the same shape with the plain operand, twice (the second call may take the memoised fast
            # path), must not capture the coded call that follows
            ("plain operand", "rs", Operators.Float.SUM, counts, "plain", exact_rs(counts, torch.add), (0, 0)),
            ("plain operand again", "rs", Operators.Float.SUM, counts, "plain", exact_rs(counts, torch.add), (0, 0)),
            ("fp8 after exact", "rs", Operators.Float.SUM, counts, None, want_rs, (1, 0)),
            ("fp8", "ag", None, counts, None, want_ag, (0, 1)),
            ("fp8 again", "ag", None, counts, None, want_ag, (0, 1)),
            ("odd offsets", "ag", None, odd, None, exact_ag(odd), (0, 0)),
            ("rccl transport", "ag", None, counts, "rccl", exact_ag(counts), (0, 0)),
            ("plain operand", "ag", None, counts, "plain", exact_ag(counts), (0, 0)),
            ("plain operand again", "ag", None, counts, "plain", exact_ag(counts), (0, 0)),
            ("fp8 after exact", "ag", None, counts, None, want_ag, (0, 1)),
        ]
        for label, kind, operator, cnts, env, want, delta in checks:
            got, moved = call(kind, x, plain if env == "plain" else operand, operator, frm, cnts,
                              env if env == "rccl" else None)
            rows.append(dict(case=name, label=label, kind=kind, equal=same_bits(got, want), moved=moved, want=delta,
                             amb=amb_rs + amb_ag, ndiff=int((got != want).sum())))
    return rows


def test_fp8_operand_is_honoured_by_reduce_scatter_and_allgather():
    res = run_spawn(2, _api)
    assert sorted(res) == [0, 1]
    for r, rows in res.items():
        assert len(rows) == 30
        for row in rows:
            what = (r, row["case"], row["kind"], row["label"])
            assert row["amb"] == 0, what
            assert row["equal"], (what, row["ndiff"])
            assert tuple(row["moved"]) == tuple(row["want"]), (what, row["moved"])


# ---------------------------------------------------------------- ZeRO with compressed gradients
# Largest relative loss difference over the 6 steps between grad_codec="fp8" and the exact run,
# same p and seeds, measured once on an MI355X (2 ranks sharing the GPU): 9.274076e-04 for f32
# parameters, 2.604167e-03 for bf16 parameters (_ZERO_MEASURED).  The run is deterministic
# (rank-ordered sums, fixed seeds); the test asserts 2x the measured value, a margin that only
# covers another library build.
_ZERO_MEASURED = {"float32": 9.274076e-04, "bfloat16": 2.604167e-03}


def _zero(comm, dtype_name):
    from mp4x.models.zero import train_zero
    dtype = getattr(torch, dtype_name)
    exact = train_zero(comm, steps=6, global_batch=48, device="cuda", dtype=dtype)
    before = dict(comm.device.stats)
    losses = train_zero(comm, steps=6, global_batch=48, device="cuda", dtype=dtype, grad_codec="fp8")
    used = {k: c - before.get(k, 0) for k, c in comm.device.stats.items() if c != before.get(k, 0)}
    return losses, exact, used


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_zero_trains_with_fp8_gradients(dtype):
    import math
    out = run_spawn(2, _zero, args=(dtype,))
    for r, (losses, exact, used) in out.items():
        assert len(losses) == 6 and all(math.isfinite(v) for v in losses), losses
        assert used.get(RS, 0) >= 6, used
        assert used.get("allgather.ipc_zc", 0) >= 6, used        # the parameter path stays zero-copy and exact
        assert used.get(AG, 0) == 0, used
        rel = max(abs(a - b) / abs(b) for a, b in zip(losses, exact))
        print(f"zero fp8 gradients {dtype} rank {r}: max relative loss difference {rel:.6e}")
        assert rel <= 2 * _ZERO_MEASURED[dtype], (rel, losses, exact)
