"""Error feedback for the fp8 gradient reduce-scatter, the parts that need no GPU: what the public
API refuses (on every rank, before any collective work) and ZeroOptimizer(error_feedback=...) on
the CPU path, where no residual is kept."""
import pytest

torch = pytest.importorskip("torch")

from harness import run_ranks  # noqa: E402


class _Solo:
    def getSlaveNum(self):
        return 1

    def getRank(self):
        return 0


def _zero(**kw):
    from mp4x.models.zero import ZeroOptimizer
    return ZeroOptimizer(_Solo(), torch.nn.Linear(6, 3).parameters(), torch.optim.SGD, lr=0.1, **kw)


def test_error_feedback_needs_the_fp8_codec():
    with pytest.raises(ValueError, match="error_feedback"):
        _zero(error_feedback=True)
    z = _zero(grad_codec="fp8", error_feedback=True)
    assert z.error_feedback and all(b.residual is None for b in z.buckets)     # CPU, one rank: nothing kept


def test_state_dict_keys_depend_on_the_option():
    assert sorted(_zero().state_dict()) == ["masters", "optim", "p", "rank"]
    assert sorted(_zero(grad_codec="fp8").state_dict()) == ["masters", "optim", "p", "rank"]
    z = _zero(grad_codec="fp8", error_feedback=True)
    sd = z.state_dict()
    assert sorted(sd) == ["masters", "optim", "p", "rank", "residuals"] and sd["residuals"] == []
    z.load_state_dict(sd)
    del sd["residuals"]
    z.load_state_dict(sd)                                                      # a checkpoint without them loads


def _refusals(comm):
    from mp4x import Operands, Operators
    from mp4x.exceptions import Mp4jException
    p = comm.getSlaveNum()
    x = torch.ones(8 * p)
    res = torch.zeros(8 * p)
    counts = [8] * p
    out = []
    for label, operand, operator in [
        ("plain operand", Operands.FLOAT_OPERAND(), Operators.Float.SUM),
        ("max", Operands.FLOAT_OPERAND(codec="fp8"), Operators.Float.MAX),
        ("cpu tensor", Operands.FLOAT_OPERAND(codec="fp8"), Operators.Float.SUM),
    ]:
        for name in ("reduceScatterArray", "reduce_scatter_array"):
            try:
                getattr(comm, name)(x.clone(), operand, operator, 0, counts, residual=res)
                out.append((label, name, None))
            except Mp4jException as e:
                out.append((label, name, str(e)))
    # nothing collective ran: the ranks are still in step, and the exact call is unchanged
    y = torch.full((8 * p,), float(comm.getRank() + 1))
    comm.reduceScatterArray(y, Operands.FLOAT_OPERAND(codec="fp8"), Operators.Float.SUM, 0, counts)
    r = comm.getRank()
    return out, y[8 * r:8 * (r + 1)].tolist(), res.tolist()


def test_residual_keyword_is_refused_on_every_rank():
    res, _, _ = run_ranks(2, _refusals, timeout=120)
    assert sorted(res) == [0, 1]
    want = {"plain operand": "codec='fp8'", "max": "SUM", "cpu tensor": "GPU tensor"}
    for r, (rows, mine, resid) in res.items():
        assert len(rows) == 6
        for label, name, msg in rows:
            assert msg is not None and want[label] in msg, (r, label, name, msg)
        assert mine == [3.0] * 8 and resid == [0.0] * 16


def _zero_cpu(comm, ef):
    from mp4x.models.zero import train_zero
    return train_zero(comm, steps=4, global_batch=48, grad_codec="fp8", error_feedback=ef)


def test_error_feedback_is_a_no_op_without_a_gpu():
    off, _, _ = run_ranks(2, _zero_cpu, (False,), timeout=120)
    on, _, _ = run_ranks(2, _zero_cpu, (True,), timeout=120)
    for r in off:
        assert on[r] == off[r]
