"""ExpertParallelMoE on host tensors (gloo, p = 2): per-step loss parity with a single-process model
that holds every expert, and the autograd functions' gradients against the contract."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import moe_model_ref  # noqa: E402
from harness import run_ranks  # noqa: E402


def _train(comm):
    return moe_model_ref.train(comm, "cpu")


def _gradients(comm):
    return moe_model_ref.gradients(comm, "cpu")


def test_loss_parity_with_the_single_process_model():
    res, _, _ = run_ranks(2, _train, timeout=120)
    assert sorted(res) == [0, 1]
    losses = np.mean([res[r][0] for r in (0, 1)], axis=0)
    assert len(losses) == moe_model_ref.STEPS
    for r in (0, 1):
        np.testing.assert_allclose(losses, res[r][1], rtol=1e-5, atol=1e-7)
        assert res[r][2] < 1e-5, (r, res[r][2])
    assert losses[-1] < losses[0]                                # ... and it trains


@pytest.mark.parametrize("p", [2, 3])
def test_backward_passes_equal_the_contract(p):
    res, _, _ = run_ranks(p, _gradients, timeout=120)
    assert sorted(res) == list(range(p))
    for r, row in res.items():
        assert row["out"], r
        assert row["dispatch"], r                                # bit for bit: the combine kernel's path
        assert row["rows"], r                                    # bit for bit: the route scatter's path
        assert row["weights"], (r, row["worst"])
