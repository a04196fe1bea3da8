"""ExpertParallelMoE(source_capacity=) on the GPU (2 processes sharing cuda:0): per-step loss parity
with the per-source first-come single-process model, and the autograd functions' gradients in the
padded layout, which run the padded K9 scatter (with ``row_scale`` in the combine's backward) and the
combine over padded slots, bit for bit against the contract."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import moe_model_ref  # noqa: E402
import moe_padded_ref as pad  # noqa: E402
from spawn_ranks import run_spawn  # noqa: E402

pytestmark = pytest.mark.gpu


def _both(comm):
    return pad.train(comm, "cuda"), pad.gradients(comm, "cuda"), dict(comm.device.stats)


def test_training_and_gradients_in_the_padded_layout_on_the_gpu():
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
        assert grads["cut_weights"], r
        assert grads["n_cut"] == grads["plan_cut"] == grads["want_cut"], (r, grads)
        # 5 steps (dispatch; combine + its backward's dispatch) and the gradient check's two of each
        assert stats["moe.dispatch"] == 2 * moe_model_ref.STEPS + 2, (r, stats)
        assert stats["moe.combine"] == moe_model_ref.STEPS + 2, (r, stats)
        assert stats["all_to_all_v.ipc.padded"] == stats["moe.dispatch"] + stats["moe.combine"], (r, stats)
        assert stats["moe.dispatch.padded"] == moe_model_ref.STEPS + 1 and "all_to_all_v.ipc" not in stats, (r, stats)
    pad.check_plans({r: res[r][0] for r in (0, 1)}, 2)
