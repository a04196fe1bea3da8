"""dispatchTokens(sourceCapacity=) / combineTokens through the public API on the GPU (p processes
sharing cuda:0).  Eager: the (case, S) table of tests/moe_padded_ref.py, dispatch -> integer "experts"
-> combine, bit for bit against the definition; one IPC copy plan per dispatch and per combine and no
count exchange at all; the inputs untouched.  Captured: the same step recorded once by
``comm.device.capture`` and replayed on fresh tokens, ids and weights in the same tensors."""
import pytest

torch = pytest.importorskip("torch")

import moe_padded_ref as pad  # noqa: E402
import moe_ref  # noqa: E402
from moe_ref import same_bits  # noqa: E402
from spawn_ranks import run_spawn  # noqa: E402

pytestmark = pytest.mark.gpu

IPC = ("all_to_all_v.ipc", "all_to_all_v.ipc.padded")


def _moved(stats, before):
    return {k: c - before.get(k, 0) for k, c in stats.items() if c != before.get(k, 0)}


def _factors(first_expert, el):
    return torch.tensor([moe_ref.expert_factor(first_expert + e) for e in range(el)], dtype=torch.float32, device="cuda")


def _device_experts(rows, factors):
    """moe_ref's integer experts on the padded layout, on the device (exact in every dtype used)."""
    return (rows.to(torch.float32) * factors.view((-1,) + (1,) * (rows.dim() - 1))).to(rows.dtype)


def _api(comm):
    from mp4x.parallel import sparse
    r, p = comm.getRank(), comm.getSlaveNum()
    stats = comm.device.stats
    out = []
    gathers, gather = [], sparse._count_matrix
    sparse._count_matrix = lambda *a: gathers.append(1) or gather(*a)
    try:
        for name, S in pad.TABLE:
            want = pad.end_to_end(name, p, S)[r]
            E, el = want["E"], want["E"] // p
            x, ids, w = want["x"].to("cuda"), want["ids"].to("cuda"), want["w"].to("cuda")
            before = dict(stats)
            rows, plan = comm.dispatchTokens(x, ids, E, sourceCapacity=S)
            torch.cuda.synchronize()
            d_used = _moved(stats, before)
            y = _device_experts(rows, _factors(r * el, el))
            before = dict(stats)
            got, back = comm.combineTokens(y, plan, w, returnSlotRows=True)
            torch.cuda.synchronize()
            c_used = _moved(stats, before)
            again = comm.combine_tokens(y, plan, w)
            out.append(dict(name=(name, S), shape=tuple(rows.shape) == (el, p * S) + tuple(x.shape[1:]),
                            rows=same_bits(rows, want["rows"]),
                            pads=pad.pads_are_zero_bits(rows.cpu(), plan.valid.cpu(), S),
                            slots=torch.equal(plan.slots.cpu(), want["slots"]),
                            kept=torch.equal(plan.kept.cpu(), want["kept"]),
                            valid=torch.equal(plan.valid.cpu(), want["valid"]),
                            dropped=torch.equal(plan.dropped.cpu(), want["dropped"]),
                            on_device=plan.kept.is_cuda and plan.valid.is_cuda and plan.dropped.is_cuda,
                            back=same_bits(back, want["back"]), out=same_bits(got, want["out"]),
                            again=same_bits(again, got),
                            plan=plan.source_capacity == S and plan.expert_counts == (p * S,) * el
                            and plan.send_counts == plan.recv_counts == (el * S,) * p and plan.clipped is None
                            and plan.demand_matrix is None and plan.expert_matrix is None,
                            untouched=same_bits(x, want["x"]) and torch.equal(ids.cpu(), want["ids"])
                            and same_bits(w, want["w"]),
                            d_used=d_used, c_used=c_used, gathers=len(gathers)))
    finally:
        sparse._count_matrix = gather
    return out


@pytest.mark.parametrize("p", [2, 3])
def test_the_table_through_the_public_api(p):
    res = run_spawn(p, _api)
    assert sorted(res) == list(range(p))
    for r, rows in res.items():
        assert [row["name"] for row in rows] == pad.TABLE
        for row in rows:
            what = (r, row["name"])
            for key in ("shape", "rows", "pads", "slots", "kept", "valid", "dropped", "on_device", "back", "out", "again",
                        "plan", "untouched"):
                assert row[key], (what, key)
            d, c = row["d_used"], row["c_used"]
            assert d.get("moe.dispatch") == 1 and d.get("moe.dispatch.padded") == 1, (what, d)
            assert sum(d.get(k, 0) for k in IPC) == 1 and sum(c.get(k, 0) for k in IPC) == 1, (what, d, c)
            assert c.get("moe.combine") == 1 and "moe.combine" not in d and "moe.dispatch" not in c, (what, d, c)
            assert row["gathers"] == 0, what


def _other_transports(comm):
    """The same call where the copy plan does not run: with an operand (the exact all-to-all with the
    constant matrix, then the counts) and, MP4X_SPARSE_IPC=0, the two equal-split all-to-alls."""
    from mp4x import Operands
    r, p = comm.getRank(), comm.getSlaveNum()
    stats = comm.device.stats
    out = []
    for name, S, operand in (("A", 40, Operands.FLOAT_OPERAND()), ("D", 100, None), ("B", 3, None)):
        want = pad.end_to_end(name, p, S)[r]
        E, el = want["E"], want["E"] // p
        x, ids, w = want["x"].to("cuda"), want["ids"].to("cuda"), want["w"].to("cuda")
        before = dict(stats)
        rows, plan = comm.dispatchTokens(x, ids, E, operand=operand, sourceCapacity=S)
        got = comm.combineTokens(_device_experts(rows, _factors(r * el, el)), plan, w, operand=operand)
        out.append(dict(name=(name, S), rows=same_bits(rows, want["rows"]), out=same_bits(got, want["out"]),
                        valid=torch.equal(plan.valid.cpu(), want["valid"]), kept=torch.equal(plan.kept.cpu(), want["kept"]),
                        used=_moved(stats, before)))
    return out


def test_the_operand_goes_to_the_exact_all_to_all():
    res = run_spawn(2, _other_transports)
    for r, rows in res.items():
        for row in rows:
            assert row["rows"] and row["out"] and row["valid"] and row["kept"], (r, row)
        used = rows[0]["used"]                                    # with the operand: the ragged transport's kernel
        assert used.get("all_to_all_v.ipc") == 2 and "all_to_all_v.ipc.padded" not in used, (r, used)
        assert rows[1]["used"].get("all_to_all_v.ipc.padded") == 2, (r, rows[1]["used"])


def test_without_the_mesh_two_equal_split_all_to_alls():
    res = run_spawn(2, _other_transports, env={"MP4X_SPARSE_IPC": "0"})
    for r, rows in res.items():
        for row in rows:
            assert row["rows"] and row["out"] and row["valid"] and row["kept"], (r, row)
            assert not any(k.startswith("all_to_all_v.ipc") for k in row["used"]), (r, row["used"])


# ---------------------------------------------------------------- captured
T, K, EL, WIDTH, S = 70, 2, 2, 8, 12


def _variant(v, r, p):
    """(x, ids, w) of rank r for replay v: uniform ids with drops; nearly everything to one expert (cut
    hard); few tokens' worth of distinct experts (nothing cut)."""
    E = EL * p
    g = torch.Generator().manual_seed(7000 + 10 * v + r)
    if v % 3 == 0:
        ids = torch.randint(-1, E, (T, K), generator=g)
    elif v % 3 == 1:
        ids = torch.where(torch.rand(T, K, generator=g) < 0.8, torch.full((T, K), (r + 1) % E),
                          torch.randint(0, E, (T, K), generator=g))
    else:
        ids = torch.full((T, K), -1)
        ids[:S // 2] = torch.randint(0, E, (S // 2, K), generator=g)
    return moe_ref.tokens(T, WIDTH, torch.float32, 7100 + 10 * v + r), ids, moe_ref.gate_weights(T, K, 7200 + 10 * v + r)


def _captured(comm):
    from mp4x.parallel import sparse
    r, p = comm.getRank(), comm.getSlaveNum()
    E = EL * p
    x = torch.zeros(T, WIDTH, device="cuda")
    ids = torch.zeros(T, K, dtype=torch.int64, device="cuda")
    w = torch.zeros(T, K, device="cuda")
    out = torch.zeros(T, WIDTH, device="cuda")
    state, factors = {}, _factors(r * EL, EL)

    def load(v):
        xv, iv, wv = _variant(v, r, p)
        x.copy_(xv)
        ids.copy_(iv)
        w.copy_(wv)

    def step():
        rows, plan = comm.dispatchTokens(x, ids, E, sourceCapacity=S)
        out.copy_(comm.combineTokens(_device_experts(rows, factors), plan, w))
        state["plan"] = plan

    load(0)
    gathers, gather = [], sparse._count_matrix
    sparse._count_matrix = lambda *a: gathers.append(1) or gather(*a)
    try:
        g = comm.device.capture(step)
    finally:
        sparse._count_matrix = gather
    plan = state["plan"]
    res = []
    for v in (1, 2, 3):
        load(v)
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        want = pad.from_inputs([_variant(v, i, p) + (E,) for i in range(p)], S)[r]
        res.append(dict(out=same_bits(out, want["out"]), valid=torch.equal(plan.valid.cpu(), want["valid"]),
                        kept=torch.equal(plan.kept.cpu(), want["kept"]),
                        dropped=torch.equal(plan.dropped.cpu(), want["dropped"]),
                        slots=torch.equal(plan.slots.cpu(), want["slots"]), cut=int(want["dropped"][0])))
    at_capture = int(pad.from_inputs([_variant(0, i, p) + (E,) for i in range(p)], S)[r]["dropped"][0])
    return res, at_capture, len(gathers)


def test_a_captured_step_replays_exactly_on_fresh_ids():
    res = run_spawn(2, _captured)
    assert sorted(res) == [0, 1]
    for r, (replays, at_capture, gathers) in res.items():
        assert len(replays) == 3 and gathers == 0
        for v, row in enumerate(replays):
            for key in ("out", "valid", "kept", "dropped", "slots"):
                assert row[key], (r, v, key)
        cuts = [row["cut"] for row in replays]
        assert any(c != at_capture for c in cuts) and max(cuts) > 0 and min(cuts) == 0, (r, at_capture, cuts)
