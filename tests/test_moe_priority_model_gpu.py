"""ExpertParallelMoE(drop_policy="probs") on the GPU (2 processes sharing cuda:0), tiny shapes (d = 16,
24 tokens, 4 experts, float32): the checks of tests/test_moe_priority_model.py with the K15 select in
the dispatch."""
import pytest

torch = pytest.importorskip("torch")

import moe_priority_ref as ref  # noqa: E402
from spawn_ranks import run_spawn  # noqa: E402

pytestmark = pytest.mark.gpu


def _checks(comm):
    return ref.model_checks(comm, "cuda")


def test_drop_by_gate_weight_in_the_layer_on_the_gpu():
    res = run_spawn(2, _checks)
    assert sorted(res) == [0, 1]
    ref.check_model(res, 2)
