"""ExpertParallelMoE(drop_policy="probs") on host tensors (gloo), tiny shapes: without overflow it is
``"position"`` bit for bit (output and every gradient); with overflow every expert keeps its top S by
gate weight (tests/moe_priority_ref.py); the gate weight of a dropped assignment gets gradient +0
through both combine backwards; and the constructor's refusals."""
import pytest

torch = pytest.importorskip("torch")

import moe_priority_ref as ref  # noqa: E402
from harness import run_ranks  # noqa: E402


def _checks(comm):
    return ref.model_checks(comm, "cpu")


@pytest.mark.parametrize("p", [1, 2])
def test_drop_by_gate_weight_in_the_layer(p):
    res, _, _ = run_ranks(p, _checks, timeout=120)
    assert sorted(res) == list(range(p))
    ref.check_model(res, p)


class OneRank:
    def getSlaveNum(self):
        return 1

    def getRank(self):
        return 0


def test_the_constructor_refuses():
    from mp4x.models.moe import ExpertParallelMoE
    with pytest.raises(ValueError, match="drop_policy"):
        ExpertParallelMoE(OneRank(), 4, 4, 2, 1, drop_policy="probs")                    # nothing is dropped
    with pytest.raises(ValueError, match="drop_policy"):
        ExpertParallelMoE(OneRank(), 4, 4, 2, 1, source_capacity=2, drop_policy="weights")
    with pytest.raises(ValueError, match="drop_policy"):
        ExpertParallelMoE(OneRank(), 4, 4, 2, 1, capacity_factor=1.0, drop_policy=None)
    for kw in (dict(source_capacity=2), dict(capacity_factor=1.0)):
        assert ExpertParallelMoE(OneRank(), 4, 4, 2, 1, drop_policy="probs", **kw).drop_policy == "probs"
    assert ExpertParallelMoE(OneRank(), 4, 4, 2, 1).drop_policy == "position"
