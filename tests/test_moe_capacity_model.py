"""ExpertParallelMoE(capacity_factor=) and the autograd functions under a capacity on host tensors
(gloo): per-step loss parity with a single-process model that drops by the same first-come rule over
the rank-major concatenation, and the gradients against the contract computed from the clipped ids
(tests/moe_capacity_ref.py)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import moe_capacity_ref as cap  # noqa: E402
import moe_model_ref  # noqa: E402
from harness import run_ranks  # noqa: E402


def _train(comm):
    return cap.train(comm, "cpu")


def _gradients(comm):
    return cap.gradients(comm, "cpu")


def test_loss_parity_with_the_capped_single_process_model():
    res, _, _ = run_ranks(2, _train, timeout=120)
    assert sorted(res) == [0, 1]
    losses = np.mean([res[r][0] for r in (0, 1)], axis=0)
    assert len(losses) == moe_model_ref.STEPS
    for r in (0, 1):
        np.testing.assert_allclose(losses, res[r][1], rtol=1e-5, atol=1e-7)
        assert res[r][2] < 1e-5, (r, res[r][2])
    cap.check_plans(res, 2)


@pytest.mark.parametrize("p", [2, 3])
def test_backward_passes_equal_the_contract_of_the_clipped_ids(p):
    res, _, _ = run_ranks(p, _gradients, timeout=120)
    assert sorted(res) == list(range(p))
    for r, row in res.items():
        assert row["slots"] and row["out"], r
        assert row["dispatch"], r                                # bit for bit: the combine's path
        assert row["rows"], r                                    # bit for bit: the route scatter along the clipping
        assert row["weights"], (r, row["worst"])
        assert row["clipped_weights"], r                         # exactly 0 for a clipped assignment
        assert row["n_clipped"] == row["plan_clipped"] == row["want_clipped"], (r, row)
    assert sum(row["n_clipped"] for row in res.values()) > 0
