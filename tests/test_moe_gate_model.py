"""ExpertParallelMoE(router="fused", renormalize=True, aux_loss_coef, z_loss_coef) on host tensors
(gloo, p = 2): per-step loss parity with a single-process model that holds every expert and computes
the same router and the same two auxiliary losses per rank with plain torch autograd
(tests/moe_gate_ref.py), at the sizes and tolerances of the GPU model test; and the default router
untouched."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import moe_gate_ref  # noqa: E402
from harness import run_ranks  # noqa: E402
from moe_model_ref import STEPS  # noqa: E402


def _train(comm):
    return moe_gate_ref.train(comm, "cpu")


def _default(comm):
    return moe_gate_ref.default_untouched(comm, "cpu")


def test_loss_parity_with_the_single_process_model():
    res, _, _ = run_ranks(2, _train, timeout=120)
    assert sorted(res) == [0, 1]
    losses = np.mean([res[r][0] for r in (0, 1)], axis=0)
    assert len(losses) == STEPS
    for r in (0, 1):
        mine, whole, drift, aux_only, aux_err = res[r]
        np.testing.assert_allclose(losses, whole, rtol=1e-4, atol=1e-6)
        assert drift < 1e-4, (r, drift)
        assert aux_only > 0 and aux_err < 1e-6 * max(1.0, aux_only), (r, aux_only, aux_err)
    assert losses[-1] < losses[0]


def test_the_default_router_is_the_layer_as_it_was():
    res, _, _ = run_ranks(2, _default, timeout=120)
    for r, row in res.items():
        assert row["kind"] == "torch" and row["calls"] == 0 and row["aux"], (r, row)
        assert row["route"] and row["out"], (r, row)


def test_the_constructor_refuses_what_the_default_router_cannot_do():
    from mp4x.models.moe import ExpertParallelMoE

    class OneRank:
        def getSlaveNum(self):
            return 1

        def getRank(self):
            return 0
    for kw in (dict(router="triton"), dict(renormalize=True), dict(aux_loss_coef=0.1), dict(z_loss_coef=0.1)):
        with pytest.raises(ValueError):
            ExpertParallelMoE(OneRank(), 8, 8, 2, 1, **kw)
