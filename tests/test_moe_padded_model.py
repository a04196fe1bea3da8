"""ExpertParallelMoE(source_capacity=) and the autograd functions in the padded layout on host tensors
(gloo): per-step loss parity with a single-process model that drops by the same per-source first-come
rule (it is given the per-rank batches), and the gradients against the contract of
tests/moe_padded_ref.py."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import moe_model_ref  # noqa: E402
import moe_padded_ref as pad  # noqa: E402
from harness import run_ranks  # noqa: E402


def _train(comm):
    return pad.train(comm, "cpu")


def _gradients(comm):
    return pad.gradients(comm, "cpu")


def test_loss_parity_with_the_per_source_single_process_model():
    res, _, _ = run_ranks(2, _train, timeout=120)
    assert sorted(res) == [0, 1]
    losses = np.mean([res[r][0] for r in (0, 1)], axis=0)
    assert len(losses) == moe_model_ref.STEPS
    for r in (0, 1):
        np.testing.assert_allclose(losses, res[r][1], rtol=1e-5, atol=1e-7)
        assert res[r][2] < 1e-5, (r, res[r][2])
    pad.check_plans(res, 2)


@pytest.mark.parametrize("p", [2, 3])
def test_backward_passes_equal_the_contract_of_the_padded_layout(p):
    res, _, _ = run_ranks(p, _gradients, timeout=120)
    assert sorted(res) == list(range(p))
    for r, row in res.items():
        assert row["slots"] and row["out"], r
        assert row["dispatch"], r                                # bit for bit: the combine's path
        assert row["rows"], r                                    # bit for bit: the padded scatter, pads zero
        assert row["weights"], (r, row["worst"])
        assert row["cut_weights"], r                             # exactly 0 for a cut assignment
        assert row["n_cut"] == row["plan_cut"] == row["want_cut"], (r, row)
    assert sum(row["n_cut"] for row in res.values()) > 0


def test_the_layer_refuses_both_capacities():
    from mp4x.models.moe import ExpertParallelMoE

    class OneRank:
        def getSlaveNum(self):
            return 1

        def getRank(self):
            return 0
    with pytest.raises(ValueError):
        ExpertParallelMoE(OneRank(), 4, 4, 2, 1, capacity_factor=1.0, source_capacity=2)
