"""ExpertParallelMoE(capacity_factor=) on the GPU (2 processes sharing cuda:0): per-step loss parity
with the capped single-process model, and the autograd functions' gradients under a capacity, which
run the clipped K9 scatter (with ``row_scale`` in the combine's backward), bit for bit against the
contract of the clipped ids."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import moe_capacity_ref as cap  # noqa: E402
import moe_model_ref  # noqa: E402
from spawn_ranks import run_spawn  # noqa: E402

pytestmark = pytest.mark.gpu


def _both(comm):
    return cap.train(comm, "cuda"), cap.gradients(comm, "cuda"), dict(comm.device.stats)


def test_training_and_gradients_under_a_capacity_on_the_gpu():
    res = run_spawn(2, _both)
    assert sorted(res) == [0, 1]
    losses = np.mean([res[r][0][0] for r in (0, 1)], axis=0)
    assert len(losses) == moe_model_ref.STEPS
    for r in (0, 1):
        (_, whole, drift, _), grads, stats = res[r]
        print(f"rank {r}: max relative loss difference {np.max(np.abs(losses - whole) / np.abs(whole)):.3e}, "
              f"drift {drift:.3e}")
        np.testing.assert_allclose(losses, whole, rtol=1e-5, atol=1e-7)
        assert drift < 1e-5, (r, drift)
        assert grads["slots"] and grads["out"] and grads["dispatch"] and grads["rows"], (r, grads)
        assert grads["weights"], (r, grads["worst"])
        assert grads["clipped_weights"], r
        assert grads["n_clipped"] == grads["plan_clipped"] == grads["want_clipped"], (r, grads)
        # 5 steps (dispatch; combine + its backward's dispatch) and the gradient check's two of each
        assert stats["moe.dispatch"] == 2 * moe_model_ref.STEPS + 2, (r, stats)
        assert stats["moe.combine"] == moe_model_ref.STEPS + 2, (r, stats)
        assert stats["all_to_all_v.ipc"] == stats["moe.dispatch"] + stats["moe.combine"], (r, stats)
    cap.check_plans({r: res[r][0] for r in (0, 1)}, 2)
