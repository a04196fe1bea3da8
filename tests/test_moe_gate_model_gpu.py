"""ExpertParallelMoE(router="fused") on the GPU (2 processes sharing cuda:0), where the router is the
K10 kernels: per-step loss parity with the single-process model of tests/moe_gate_ref.py (the same
router and the same two auxiliary losses per rank in plain torch autograd), the auxiliary losses
alone reaching the router's gradient (``g_psum`` and ``g_lse`` reach the kernel), the default router
untouched, and a captured step router -> dispatchTokens(sourceCapacity=S) -> experts -> combineTokens
replayed on fresh logits."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import moe_gate_ref  # noqa: E402
import moe_ref  # noqa: E402
from moe_model_ref import STEPS  # noqa: E402
from moe_ref import same_bits  # noqa: E402
from spawn_ranks import run_spawn  # noqa: E402

pytestmark = pytest.mark.gpu


def _model(comm):
    from mp4x.ops import device_ops
    calls = {"fwd": 0, "bwd": 0}
    fwd, bwd = device_ops.moe_gate_topk, device_ops.moe_gate_backward

    def count(name, f):
        def g(*a, **k):
            calls[name] += 1
            return f(*a, **k)
        return g
    device_ops.moe_gate_topk, device_ops.moe_gate_backward = count("fwd", fwd), count("bwd", bwd)
    try:
        default = moe_gate_ref.default_untouched(comm, "cuda")
        untouched = dict(calls)
        trained = moe_gate_ref.train(comm, "cuda")
    finally:
        device_ops.moe_gate_topk, device_ops.moe_gate_backward = fwd, bwd
    return trained, default, untouched, calls


def test_training_with_the_fused_router_and_the_default_untouched():
    res = run_spawn(2, _model)
    assert sorted(res) == [0, 1]
    losses = np.mean([res[r][0][0] for r in (0, 1)], axis=0)
    assert len(losses) == STEPS
    for r in (0, 1):
        (_, whole, drift, aux_only, aux_err), default, untouched, calls = res[r]
        np.testing.assert_allclose(losses, whole, rtol=1e-4, atol=1e-6)
        assert drift < 1e-4, (r, drift)
        assert aux_only > 0 and aux_err < 1e-6 * max(1.0, aux_only), (r, aux_only, aux_err)
        # the K10 kernels ran: the auxiliary-only step and the 5 training steps, forward and backward
        assert calls == {"fwd": STEPS + 1, "bwd": STEPS + 1}, (r, calls)
        assert untouched == {"fwd": 0, "bwd": 0}, (r, untouched)
        assert default["kind"] == "torch" and default["calls"] == 0 and default["aux"], (r, default)
        assert default["route"] and default["out"], (r, default)
    assert losses[-1] < losses[0]


# ---------------------------------------------------------------- captured
T, K, EL, WIDTH, S = 70, 2, 2, 8, 12


def _variant(v, r, p):
    """(x, logits) of rank r for step v.  0, the captured one: uniform logits, every expert over its
    share; 1: one expert far ahead and one far behind but for a few tokens; 2: integer logits full of
    ties, the last two experts masked (-inf) but for 5 tokens; 3: uniform, expert 0 masked but for 7."""
    E = EL * p
    lg = moe_gate_ref.uniform_logits(T, E, 4 if v != 1 else 1, 8000 + 10 * v + r)
    if v == 1:
        lg[:, (r + 1) % E] += 8.0
        lg[S // 2:, (r + 2) % E] -= 8.0
    elif v == 2:
        lg = torch.randint(-2, 3, (T, E), generator=torch.Generator().manual_seed(8000 + 10 * v + r)).to(torch.float32)
        lg[5:, E - 2:] = float("-inf")
    elif v == 3:
        lg[7:, 0] = float("-inf")
    return moe_ref.tokens(T, WIDTH, torch.float32, 8100 + 10 * v + r), lg


def _captured(comm):
    from mp4x.models.moe import route_topk
    from mp4x.parallel import sparse
    r, p = comm.getRank(), comm.getSlaveNum()
    E = EL * p
    x = torch.zeros(T, WIDTH, device="cuda")
    logits = torch.zeros(T, E, device="cuda")
    out = torch.zeros(T, WIDTH, device="cuda")
    factors = torch.tensor([moe_ref.expert_factor(r * EL + e) for e in range(EL)], dtype=torch.float32, device="cuda")
    state = {}

    def load(v):
        xv, lv = _variant(v, r, p)
        x.copy_(xv)
        logits.copy_(lv)

    def step():
        gate = route_topk(logits, K, renormalize=True)
        rows, plan = comm.dispatchTokens(x, gate.ids, E, sourceCapacity=S)
        y = (rows * factors.view(-1, 1, 1)).to(rows.dtype)
        out.copy_(comm.combineTokens(y, plan, gate.weights))
        state["plan"], state["ids"] = plan, gate.ids

    def snapshot():
        torch.cuda.synchronize()
        plan = state["plan"]
        return out.clone().cpu(), plan.kept.cpu().clone(), plan.dropped.cpu().clone(), state["ids"].cpu().clone()

    eager = {}
    for v in (0, 1, 2, 3):                          # the eager results first: after the capture only replays run
        load(v)
        out.fill_(float("nan"))
        step()
        eager[v] = snapshot()
    load(0)
    gathers, gather = [], sparse._count_matrix
    sparse._count_matrix = lambda *a: gathers.append(1) or gather(*a)
    try:
        g = comm.device.capture(step)
    finally:
        sparse._count_matrix = gather
    res = []
    for v in (1, 2, 3):
        load(v)
        out.fill_(float("nan"))
        g.replay()
        got = snapshot()
        want_ids = moe_gate_ref.order_ids(_variant(v, r, p)[1], K)
        res.append(dict(out=same_bits(got[0], eager[v][0]), finite=bool(torch.isfinite(got[0]).all()),
                        kept=torch.equal(got[1], eager[v][1]), dropped=torch.equal(got[2], eager[v][2]),
                        ids=torch.equal(got[3], eager[v][3]) and torch.equal(got[3], want_ids),
                        plan=(got[1].tolist(), got[2].tolist())))
    return res, (eager[0][1].tolist(), eager[0][2].tolist()), len(gathers)


def test_a_captured_step_from_the_router_replays_exactly_on_fresh_logits():
    res = run_spawn(2, _captured)
    assert sorted(res) == [0, 1]
    for r, (replays, at_capture, gathers) in res.items():
        assert len(replays) == 3 and gathers == 0
        for v, row in enumerate(replays):
            for key in ("out", "finite", "kept", "dropped", "ids"):
                assert row[key], (r, v, key)
        plans = [row["plan"] for row in replays]
        assert all(pl != at_capture for pl in plans), (r, at_capture, plans)       # kept / dropped moved with the logits
        assert len({str(pl) for pl in plans}) == 3, (r, plans)
