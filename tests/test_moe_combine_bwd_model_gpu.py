"""ExpertParallelMoE(combine_backward="fused") on the GPU (2 processes sharing cuda:0), where the
combine's backward is the K11 kernel: the training loops of tests/moe_model_ref.py and of its capped
and padded forms, with per-step loss parity with their single-process models at those tests'
tolerances and one K11 launch per step; and the default model, which never launches it and whose
gradients are bit-equal to the parent's code path (``_Combine`` with ``backward="torch"``)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import moe_model_ref  # noqa: E402
from moe_model_ref import STEPS  # noqa: E402
from moe_ref import same_bits  # noqa: E402
from spawn_ranks import run_spawn  # noqa: E402

pytestmark = pytest.mark.gpu


def _counted(fn):
    """``fn()`` with ``device_ops.moe_combine_backward`` counted: (result, calls)."""
    from mp4x.ops import device_ops
    calls, real = [0], device_ops.moe_combine_backward

    def counting(*a, **k):
        calls[0] += 1
        return real(*a, **k)
    device_ops.moe_combine_backward = counting
    try:
        return fn(), calls[0]
    finally:
        device_ops.moe_combine_backward = real


def _fused(comm, which):
    """The training loop ``which`` with every model it builds given ``combine_backward="fused"``."""
    import moe_capacity_ref
    import moe_padded_ref
    from mp4x.models import moe
    train = {"plain": moe_model_ref.train, "capacity": moe_capacity_ref.train, "padded": moe_padded_ref.train}[which]
    real = moe.ExpertParallelMoE

    class Fused(real):
        def __init__(self, *a, **k):
            super().__init__(*a, combine_backward="fused", **k)
    moe.ExpertParallelMoE = Fused
    try:
        res, calls = _counted(lambda: train(comm, "cuda"))
    finally:
        moe.ExpertParallelMoE = real
    return res[:3], calls, dict(comm.device.stats)


# which -> (rtol, atol, drift) of the existing GPU test of that loop
TOLERANCES = {"plain": (1e-4, 1e-6, 1e-4), "capacity": (1e-5, 1e-7, 1e-5), "padded": (1e-5, 1e-7, 1e-5)}


@pytest.mark.parametrize("which", sorted(TOLERANCES))
def test_training_with_the_fused_combine_backward(which):
    res = run_spawn(2, _fused, args=(which,), timeout=120)
    assert sorted(res) == [0, 1]
    rtol, atol, max_drift = TOLERANCES[which]
    losses = np.mean([res[r][0][0] for r in (0, 1)], axis=0)
    assert len(losses) == STEPS
    for r in (0, 1):
        (_, whole, drift), calls, stats = res[r]
        print(f"{which} rank {r}: max relative loss difference {np.max(np.abs(losses - whole) / np.abs(whole)):.3e}, "
              f"drift {drift:.3e}")
        np.testing.assert_allclose(losses, whole, rtol=rtol, atol=atol)
        assert drift < max_drift, (r, drift)
        assert calls == STEPS, (r, calls)                                   # K11 once per step
        assert stats["moe.combine.backward"] == STEPS, (r, stats)
        assert stats["moe.dispatch"] == STEPS and stats["moe.combine"] == STEPS, (r, stats)         # no second dispatch
    assert losses[-1] < losses[0]


def _default(comm):
    """One step of the default model, then the same step with the layer's combine replaced by a direct
    ``_Combine.apply(..., "torch")``: the parent's code path in this process."""
    from mp4x.models import moe
    m, r = moe_model_ref, comm.getRank()
    x, y = (t.to("cuda") for t in m.batch(r))

    def step():
        model = moe.ExpertParallelMoE(comm, m.D_MODEL, m.D_HIDDEN, m.EXPERTS, m.TOP_K, seed=m.SEED, device="cuda")
        loss = ((model(x) - y) ** 2).mean()
        loss.backward()
        return model.combine_backward, float(loss.detach()), [p.grad.detach().cpu() for p in model.parameters()]

    (kind, loss, grads), calls = _counted(step)
    real = moe.combine_tokens
    moe.combine_tokens = lambda comm_, rows, plan, w=None, operand=None, backward="torch": \
        moe._Combine.apply(rows, w, comm_, plan, operand, "torch")
    try:
        (_, parent_loss, parent), parent_calls = _counted(step)
    finally:
        moe.combine_tokens = real
    return dict(kind=kind, calls=calls + parent_calls, loss=loss == parent_loss, n=len(grads),
                grads=all(same_bits(a, b) for a, b in zip(grads, parent)),
                some=all(bool((g != 0).any()) for g in grads), counter=comm.device.stats.get("moe.combine.backward", 0))


def test_the_default_model_is_the_parents_path():
    res = run_spawn(2, _default, timeout=120)
    assert sorted(res) == [0, 1]
    for r, row in res.items():
        assert row["kind"] == "torch" and row["calls"] == 0 and row["counter"] == 0, (r, row)
        assert row["loss"] and row["grads"] and row["some"] and row["n"] == 5, (r, row)
