"""ExpertParallelMoE with the group-limited gate on the GPU (2 processes sharing cuda:0), where the
router is the K13 kernels: per-step loss parity with the single-process model of
tests/moe_gate_group_ref.py (the same router in plain torch autograd), the selection bias after
every ``update_balance_bias``, the layer without the new arguments untouched with both routers, and
a captured step grouped gate -> dispatchTokens(sourceCapacity=S) -> experts -> combineTokens replayed
on fresh logits."""
import pytest

torch = pytest.importorskip("torch")

import moe_gate_group_ref as ref  # noqa: E402
import moe_gate_ref  # noqa: E402
import moe_ref  # noqa: E402
from moe_model_ref import STEPS  # noqa: E402
from moe_ref import same_bits  # noqa: E402
from spawn_ranks import run_spawn  # noqa: E402
from test_moe_gate_group_model import check_training  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ("moe_gate_group_topk", "moe_gate_group_backward", "moe_gate_topk", "moe_gate_backward")


def _model(comm):
    from mp4x.ops import device_ops
    calls = {n: 0 for n in NAMES}
    real = {n: getattr(device_ops, n) for n in NAMES}

    def count(name):
        def g(*a, **k):
            calls[name] += 1
            return real[name](*a, **k)
        return g
    for n in NAMES:
        setattr(device_ops, n, count(n))
    try:
        default = {router: ref.default_untouched(comm, "cuda", router) for router in ("torch", "fused")}
        untouched = dict(calls)
        for n in NAMES:
            calls[n] = 0
        trained = ref.train(comm, "cuda")
    finally:
        for n in NAMES:
            setattr(device_ops, n, real[n])
    return trained, default, untouched, calls


def test_training_with_the_grouped_gate_and_the_default_untouched():
    res = run_spawn(2, _model)
    check_training({r: res[r][0] for r in res})
    for r in (0, 1):
        _, default, untouched, calls = res[r]
        # the K13 kernels ran, forward and backward, in every step, and K10's not at all
        assert calls == {NAMES[0]: STEPS, NAMES[1]: STEPS, NAMES[2]: 0, NAMES[3]: 0}, (r, calls)
        # without the new arguments: none of the new code; router="fused" is one K10 forward in the
        # layer and one in the re-evaluation
        assert untouched == {NAMES[0]: 0, NAMES[1]: 0, NAMES[2]: 2, NAMES[3]: 0}, (r, untouched)
        for router, row in default.items():
            assert row["calls"] == 0 and not row["grouped"] and row["buffers"] == [], (r, router, row)
            assert row["out"] and row["aux"], (r, router, row)


# ---------------------------------------------------------------- captured
T, K, EL, WIDTH, S, GR, KG, SCALE = 70, 2, 4, 8, 12, 4, 2, 2.5


def _variant(v, r, p):
    """(x, logits) of rank r for step v.  0, the captured one: uniform logits; 1: one expert far ahead
    and one far behind but for a few tokens; 2: small integer logits full of ties, the last group
    masked (-inf) but for 5 tokens; 3: uniform, expert 0 masked but for 7."""
    E = EL * p
    lg = moe_gate_ref.uniform_logits(T, E, 4 if v != 1 else 1, 8000 + 10 * v + r)
    if v == 1:
        lg[:, (r + 1) % E] += 8.0
        lg[S // 2:, (r + 2) % E] -= 8.0
    elif v == 2:
        lg = torch.randint(0, 5, (T, E), generator=torch.Generator().manual_seed(8000 + 10 * v + r)).to(torch.float32)
        lg[5:, E - E // GR:] = float("-inf")
    elif v == 3:
        lg[7:, 0] = float("-inf")
    return moe_ref.tokens(T, WIDTH, torch.float32, 8100 + 10 * v + r), lg


def _captured(comm):
    from mp4x.models.moe import route_topk_grouped
    from mp4x.parallel import sparse
    r, p = comm.getRank(), comm.getSlaveNum()
    E = EL * p
    x = torch.zeros(T, WIDTH, device="cuda")
    logits = torch.zeros(T, E, device="cuda")
    out = torch.zeros(T, WIDTH, device="cuda")
    bias = ref.random_bias(E, 31).to("cuda")
    factors = torch.tensor([moe_ref.expert_factor(r * EL + e) for e in range(EL)], dtype=torch.float32, device="cuda")
    state = {}

    def load(v):
        xv, lv = _variant(v, r, p)
        x.copy_(xv)
        logits.copy_(lv)

    def step():
        gate = route_topk_grouped(logits, K, score="sigmoid", bias=bias, n_group=GR, topk_group=KG, renormalize=True,
                                  scale=SCALE)
        rows, plan = comm.dispatchTokens(x, gate.ids, E, sourceCapacity=S)
        y = (rows * factors.view(-1, 1, 1)).to(rows.dtype)
        out.copy_(comm.combineTokens(y, plan, gate.weights))
        state["plan"], state["ids"], state["groups"] = plan, gate.ids, gate.group_ids

    def snapshot():
        torch.cuda.synchronize()
        plan = state["plan"]
        return (out.clone().cpu(), plan.kept.cpu().clone(), plan.dropped.cpu().clone(), state["ids"].cpu().clone(),
                state["groups"].cpu().clone())

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
        want = ref.Reference(_variant(v, r, p)[1], K, "sigmoid", bias.cpu(), GR, KG, True, SCALE)
        res.append(dict(out=same_bits(got[0], eager[v][0]), finite=bool(torch.isfinite(got[0]).all()),
                        kept=torch.equal(got[1], eager[v][1]), dropped=torch.equal(got[2], eager[v][2]),
                        ids=torch.equal(got[3], eager[v][3]) and torch.equal(got[4], eager[v][4]),
                        selection=want.selection_ok(got[4], got[3]), plan=(got[1].tolist(), got[2].tolist())))
    return res, (eager[0][1].tolist(), eager[0][2].tolist()), len(gathers)


def test_a_captured_step_from_the_grouped_gate_replays_exactly_on_fresh_logits():
    res = run_spawn(2, _captured)
    assert sorted(res) == [0, 1]
    for r, (replays, at_capture, gathers) in res.items():
        assert len(replays) == 3 and gathers == 0
        for v, row in enumerate(replays):
            for key in ("out", "finite", "kept", "dropped", "ids"):
                assert row[key], (r, v, key)
            assert row["selection"] is None, (r, v, row["selection"])
        plans = [row["plan"] for row in replays]
        assert all(pl != at_capture for pl in plans), (r, at_capture, plans)       # kept / dropped moved with the logits
        assert len({str(pl) for pl in plans}) == 3, (r, plans)
