"""ExpertParallelMoE on the GPU (2 processes sharing cuda:0): per-step loss parity with a
single-process model that holds every expert, and the autograd functions' gradients, which run the
K9 kernels, bit for bit against the contract."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import moe_model_ref  # noqa: E402
from spawn_ranks import run_spawn  # noqa: E402

pytestmark = pytest.mark.gpu


def _both(comm):
    return moe_model_ref.train(comm, "cuda"), moe_model_ref.gradients(comm, "cuda"), dict(comm.device.stats)


def test_training_and_gradients_on_the_gpu():
    res = run_spawn(2, _both)
    assert sorted(res) == [0, 1]
    losses = np.mean([res[r][0][0] for r in (0, 1)], axis=0)
    assert len(losses) == moe_model_ref.STEPS
    for r in (0, 1):
        (_, whole, drift), grads, stats = res[r]
        np.testing.assert_allclose(losses, whole, rtol=1e-4, atol=1e-6)
        assert drift < 1e-4, (r, drift)
        assert grads["out"] and grads["dispatch"] and grads["rows"], (r, grads)
        assert grads["weights"], (r, grads["worst"])
        # 5 steps (dispatch; combine + its backward's dispatch) and the gradient check's two of each
        assert stats["moe.dispatch"] == 2 * moe_model_ref.STEPS + 2, (r, stats)
        assert stats["moe.combine"] == moe_model_ref.STEPS + 2, (r, stats)
        assert stats["all_to_all_v.ipc"] == stats["moe.dispatch"] + stats["moe.combine"], (r, stats)
    assert losses[-1] < losses[0]
