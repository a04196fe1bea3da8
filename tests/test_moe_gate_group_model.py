"""ExpertParallelMoE with the group-limited gate (router="fused", score="sigmoid", expert_groups,
topk_groups, renormalize, routed_scale, balance_bias, aux_loss_coef) on host tensors (gloo, p = 2):
per-step loss parity with a single-process model that holds every expert and computes the same
router in plain torch (tests/moe_gate_group_ref.py), at the tolerances of the K10 model tests; the
selection bias after every ``update_balance_bias``; and the layer without the new arguments
untouched, with both routers."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import moe_gate_group_ref as ref  # noqa: E402
from harness import run_ranks  # noqa: E402
from moe_model_ref import STEPS  # noqa: E402


def _train(comm):
    return ref.train(comm, "cpu")


def _default(comm):
    return {router: ref.default_untouched(comm, "cpu", router) for router in ("torch", "fused")}


def check_training(res):
    assert sorted(res) == [0, 1]
    losses = np.mean([res[r][0] for r in (0, 1)], axis=0)
    assert len(losses) == STEPS
    for r in (0, 1):
        mine, whole, drift, steps, in_state = res[r]
        # the two models chose the same experts in every step: a near-tie that falls the other way
        # would be a reason to change the seed, not the tolerance
        assert all(s["same_ids"] for s in steps), (r, [s["same_ids"] for s in steps])
        np.testing.assert_allclose(losses, whole, rtol=1e-4, atol=1e-6)
        assert drift < 1e-4, (r, drift)
        assert all(s["bias_ok"] and s["in_groups"] for s in steps), (r, steps)
        assert in_state
    for a, b in zip(res[0][3], res[1][3]):
        assert a["bias"] == b["bias"]                                    # the same bits on both ranks
    assert any(v != 0 for v in res[0][3][-1]["bias"])
    assert losses[-1] < losses[0]


def test_loss_parity_and_the_balance_bias():
    res, _, _ = run_ranks(2, _train, timeout=120)
    check_training(res)


def test_without_the_new_arguments_the_layer_is_as_it_was():
    res, _, _ = run_ranks(2, _default, timeout=120)
    for r, both in res.items():
        for router, row in both.items():
            assert row["calls"] == 0 and not row["grouped"] and row["buffers"] == [], (r, router, row)
            assert row["out"] and row["aux"], (r, router, row)


def test_the_constructor_refuses():
    from mp4x.models.moe import ExpertParallelMoE

    class OneRank:
        def getSlaveNum(self):
            return 1

        def getRank(self):
            return 0
    for kw in (dict(score="sigmoid"), dict(expert_groups=2), dict(routed_scale=2.0), dict(balance_bias=True),
               dict(router="fused", score="tanh"), dict(router="fused", score="sigmoid", z_loss_coef=0.1),
               dict(router="fused", topk_groups=1),
               # what the gate itself would refuse only at the first forward
               dict(router="fused", expert_groups=3), dict(router="fused", expert_groups=0),
               dict(router="fused", expert_groups=2.0), dict(router="fused", expert_groups=True),
               dict(router="fused", expert_groups=2, topk_groups=3), dict(router="fused", expert_groups=2, topk_groups=0),
               dict(router="fused", expert_groups=4, topk_groups=1, top_k=2),
               dict(router="fused", routed_scale=0.0), dict(router="fused", routed_scale=-1.0),
               dict(router="fused", routed_scale=float("inf")), dict(router="fused", routed_scale=float("nan"))):
        kw = dict(dict(top_k=1), **kw)
        top_k = kw.pop("top_k")
        with pytest.raises(ValueError):
            ExpertParallelMoE(OneRank(), 8, 8, 4, top_k, **kw)
    model = ExpertParallelMoE(OneRank(), 8, 8, 4, 1, router="fused", score="sigmoid", expert_groups=2, topk_groups=1)
    with pytest.raises(ValueError, match="balance_bias"):
        model.update_balance_bias(0.1)
    model = ExpertParallelMoE(OneRank(), 8, 8, 4, 1, router="fused", balance_bias=True)
    with pytest.raises(ValueError, match="forward"):
        model.update_balance_bias(0.1)
    assert model.expert_bias.dtype == torch.float32 and model.expert_bias.shape == (4,)
    assert "expert_bias" in model.state_dict() and "expert_bias" not in dict(model.named_parameters())
