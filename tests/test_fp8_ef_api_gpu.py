"""reduceScatterArray(residual=...) through the public API (p = 2 processes sharing cuda:0) and
ZeroOptimizer(grad_codec="fp8", error_feedback=True) on top of it: the counters, the exact
fallbacks that leave the residual's bits alone, reproducible training, the loss against the exact
run, and a checkpoint that resumes bit for bit."""
import math
import os

import pytest

torch = pytest.importorskip("torch")

from fp8_ef_ref import ref_quant_ef  # noqa: E402
from fp8_ref import ref_dequant_reduce, ref_store  # noqa: E402
from fp8_rsag_ref import CASES, bounds, inputs, same_bits  # noqa: E402
from spawn_ranks import run_spawn  # noqa: E402

pytestmark = pytest.mark.gpu

RS, EF = "reduce_scatter.fp8.ipc", "reduce_scatter.fp8.ef"


def _api(comm):
    from mp4x import Operands, Operators
    r, p = comm.getRank(), comm.getSlaveNum()
    stats = comm.device.stats
    rows = []
    dtype_name, n, frm, counts = CASES["A"]
    counts = counts[p]
    froms, tos = bounds(frm, counts)
    xs = inputs(n, torch.float32, p)
    operand = Operands.FLOAT_OPERAND(codec="fp8")
    res0 = [torch.randn(n, generator=torch.Generator().manual_seed(40 + j)) * 1e-2 for j in range(p)]

    def call(name, cnts, env=None):
        y = xs[r].to("cuda")
        res = res0[r][:sum(cnts)].to("cuda")
        before = (stats.get(RS, 0), stats.get(EF, 0))
        old = os.environ.get("MP4X_FP8_TRANSPORT")
        if env:
            os.environ["MP4X_FP8_TRANSPORT"] = env
        try:
            getattr(comm, name)(y, operand, Operators.Float.SUM, frm, list(cnts), residual=res)
            torch.cuda.synchronize()
        finally:
            if env and old is None:
                del os.environ["MP4X_FP8_TRANSPORT"]
            elif env:
                os.environ["MP4X_FP8_TRANSPORT"] = old
        return y.cpu(), res.cpu(), (stats.get(RS, 0) - before[0], stats.get(EF, 0) - before[1])

    def exact(cnts):
        f, t = bounds(frm, cnts)
        out = xs[r].clone()
        out[f[r]:t[r]] = xs[0][f[r]:t[r]] + xs[1][f[r]:t[r]]
        return out

    # the coded call: the contract with Q_ef, both counters
    quant = [ref_quant_ef(x[froms[0]:tos[-1]], res0[j]) for j, x in enumerate(xs)]
    acc, amb = ref_dequant_reduce([t[0] for t in quant], [t[1] for t in quant])
    want = xs[r].clone()
    want[froms[r]:tos[r]] = ref_store(acc, torch.float32)[froms[r] - froms[0]:tos[r] - froms[0]]
    amb += sum(t[3] for t in quant)
    for name in ("reduceScatterArray", "reduce_scatter_array", "reduceScatterArray"):   # never memoised: the same each time
        got, res, moved = call(name, counts)
        rows.append(dict(label="fp8 ef " + name, equal=same_bits(got, want), resid=same_bits(res, quant[r][2]),
                         moved=moved, want=(1, 1), amb=amb))
    # the exact fallbacks: the plain sum, the residual's bits unchanged, no fp8 counter
    odd = [258, 510]
    for label, cnts, env in (("rccl transport", counts, "rccl"), ("odd offsets", odd, None)):
        got, res, moved = call("reduceScatterArray", cnts, env)
        rows.append(dict(label=label, equal=same_bits(got, exact(cnts)), resid=same_bits(res, res0[r][:sum(cnts)]),
                         moved=moved, want=(0, 0), amb=0))
    # a residual of the wrong size is refused on every rank, on either path
    from mp4x.exceptions import Mp4jException
    refused = 0
    for env in (None, "rccl"):
        if env:
            os.environ["MP4X_FP8_TRANSPORT"] = env
        try:
            comm.reduceScatterArray(xs[r].to("cuda"), operand, Operators.Float.SUM, frm, list(counts),
                                    residual=torch.zeros(n - 4, device="cuda"))
        except Mp4jException:
            refused += 1
        finally:
            os.environ.pop("MP4X_FP8_TRANSPORT", None)
    # a plain fp8 call afterwards is today's: one counter
    y = xs[r].to("cuda")
    before = (stats.get(RS, 0), stats.get(EF, 0))
    comm.reduceScatterArray(y, operand, Operators.Float.SUM, frm, list(counts))
    torch.cuda.synchronize()
    plain_moved = (stats.get(RS, 0) - before[0], stats.get(EF, 0) - before[1])
    return rows, refused, plain_moved


def test_residual_keyword_through_the_public_api():
    res = run_spawn(2, _api)
    assert sorted(res) == [0, 1]
    for r, (rows, refused, plain_moved) in res.items():
        assert len(rows) == 5
        for row in rows:
            what = (r, row["label"])
            assert row["amb"] == 0, what
            assert row["equal"], what
            assert row["resid"], what
            assert tuple(row["moved"]) == tuple(row["want"]), (what, row["moved"])
        assert refused == 2
        assert tuple(plain_moved) == (1, 0)


# ---------------------------------------------------------------- ZeRO with error feedback
# Largest relative loss difference over the 6 steps between grad_codec="fp8" with error_feedback
# and the exact run, same p and seeds, measured once on an MI355X (2 ranks sharing the GPU):
# _ZERO_MEASURED.  The run is deterministic (rank-ordered sums, fixed seeds); the test asserts 2x the
# measured value, the convention of tests/test_fp8_rsag_api_gpu.py for the same quantity without
# feedback (9.274e-04 / 2.604e-03 there).  Six steps say nothing about which of the two is closer;
# the deterministic evidence for error feedback is the drift case.
_ZERO_MEASURED = {"float32": 8.709063e-04, "bfloat16": 2.770083e-03}


def _zero(comm, dtype_name):
    from mp4x.models.zero import train_zero
    dtype = getattr(torch, dtype_name)
    kw = dict(steps=6, global_batch=48, device="cuda", dtype=dtype)
    exact = train_zero(comm, **kw)
    before = dict(comm.device.stats)
    first = train_zero(comm, grad_codec="fp8", error_feedback=True, **kw)
    used = {k: c - before.get(k, 0) for k, c in comm.device.stats.items() if c != before.get(k, 0)}
    second = train_zero(comm, grad_codec="fp8", error_feedback=True, **kw)
    return first, second, exact, used


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_zero_trains_with_error_feedback(dtype):
    out = run_spawn(2, _zero, args=(dtype,))
    for r, (first, second, exact, used) in out.items():
        assert len(first) == 6 and all(math.isfinite(v) for v in first), first
        assert first == second                                   # reproducible, bit for bit
        assert used.get(RS, 0) >= 6 and used.get(EF, 0) == used.get(RS, 0), used
        assert used.get("allgather.ipc_zc", 0) >= 6, used        # the parameter path stays zero-copy and exact
        rel = max(abs(a - b) / abs(b) for a, b in zip(first, exact))
        print(f"zero fp8 error feedback {dtype} rank {r}: max relative loss difference {rel:.6e}")
        assert rel <= 2 * _ZERO_MEASURED[dtype], (rel, first, exact)


def _train(comm, opt, model, steps, first_step, dtype):
    from mp4x import Operands, Operators
    from mp4x.models.mlp import synthetic_batch
    p, r = comm.getSlaveNum(), comm.getRank()
    shard = 48 // p
    losses = []
    for step in range(first_step, first_step + steps):
        x, y = synthetic_batch(step, 48, 64, 16, "cuda")
        xs, ys = x[r * shard:(r + 1) * shard].to(dtype), y[r * shard:(r + 1) * shard].to(dtype)
        opt.zero_grad()
        loss = torch.nn.functional.mse_loss(model(xs), ys)
        loss.backward()
        opt.step()
        losses.append(comm.allreduce(float(loss.detach().float().cpu()), Operands.DOUBLE_OPERAND(),
                                     Operators.Double.SUM) / p)
    return losses


def _resume(comm):
    from mp4x.models.mlp import MLP
    from mp4x.models.zero import ZeroOptimizer

    def build():
        torch.manual_seed(0)
        model = MLP(64, 128, 16).to(device="cuda")
        opt = ZeroOptimizer(comm, model.parameters(), torch.optim.AdamW, lr=0.01, weight_decay=0.01,
                            grad_codec="fp8", error_feedback=True)
        return model, opt

    model, opt = build()
    whole = _train(comm, opt, model, 6, 0, torch.float32)
    opt.close()

    model, opt = build()
    head = _train(comm, opt, model, 3, 0, torch.float32)
    sd = opt.state_dict()
    keys = sorted(sd)
    on_cpu = all(not t.is_cuda and t.dtype == torch.float32 for t in sd["residuals"])
    sizes_ok = [t.numel() for t in sd["residuals"]] == [b.n for b in opt.buckets]
    nonzero = any(bool(t.any()) for t in sd["residuals"])
    opt.close()

    model, opt = build()
    opt.load_state_dict(sd)
    tail = _train(comm, opt, model, 3, 3, torch.float32)
    bad_layout = False
    try:
        opt.load_state_dict(dict(sd, residuals=[t[:-4] for t in sd["residuals"]]))
    except ValueError:
        bad_layout = True
    opt.close()

    model, opt = build()
    for b in opt.buckets:
        b.residual.fill_(1.0)                      # must be zeroed by a checkpoint that has none
    opt.load_state_dict({k: v for k, v in sd.items() if k != "residuals"})
    zeroed = all(not bool(b.residual.any()) for b in opt.buckets)
    cold = _train(comm, opt, model, 3, 3, torch.float32)
    opt.close()
    return dict(whole=whole, head=head, tail=tail, cold=cold, keys=keys, on_cpu=on_cpu, sizes_ok=sizes_ok,
                nonzero=nonzero, bad_layout=bad_layout, zeroed=zeroed)


def test_checkpoint_resumes_bit_for_bit():
    out = run_spawn(2, _resume)
    for r, o in out.items():
        assert o["keys"] == ["masters", "optim", "p", "rank", "residuals"]
        assert o["on_cpu"] and o["sizes_ok"] and o["nonzero"], o
        assert o["head"] + o["tail"] == o["whole"], (o["head"], o["tail"], o["whole"])
        assert o["bad_layout"] and o["zeroed"]
        assert len(o["cold"]) == 3 and all(math.isfinite(v) for v in o["cold"])
