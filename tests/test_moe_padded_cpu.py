"""The padded fixed-capacity layout of dispatchTokens (sourceCapacity=S) without a GPU: host tensors
over gloo against the definition (tests/moe_padded_ref.py) and against the uncapped call, the plan's
fields, no count exchange at all, every refusal on every rank, and the native refusals of the padded
entry points on the real libmp4x_hip.so (fake pointers: the checks are host-side and launch nothing)."""
import pytest

torch = pytest.importorskip("torch")

import moe_padded_ref as pad  # noqa: E402
import moe_ref  # noqa: E402
from harness import run_ranks  # noqa: E402
from moe_ref import same_bits  # noqa: E402
from mp4x.operators import DType  # noqa: E402
from mp4x.ops import native  # noqa: E402

BADARG, UNSUPPORTED = 1001, 1002


def _counting(sparse):
    calls, gather = [], sparse._count_matrix
    sparse._count_matrix = lambda *a: calls.append(1) or gather(*a)
    return calls, gather


def _table_on_host(comm):
    from mp4x.parallel import sparse
    r, p = comm.getRank(), comm.getSlaveNum()
    stats = comm.device.stats
    out = []
    calls, gather = _counting(sparse)
    try:
        for name, S in pad.TABLE:
            want = pad.end_to_end(name, p, S)[r]
            E, el = want["E"], want["E"] // p
            x, ids, w = want["x"].clone(), want["ids"].clone(), want["w"].clone()
            before = dict(stats)
            rows, plan = comm.dispatchTokens(x, ids, E, sourceCapacity=S)
            y = pad.apply_experts(rows, r * el)
            got, back = comm.combineTokens(y, plan, w, returnSlotRows=True)
            delta = {k: stats.get(k, 0) - before.get(k, 0) for k in ("moe.dispatch", "moe.combine",
                                                                      "moe.dispatch.padded")}
            frozen = False
            try:
                plan.kept = None
            except AttributeError:
                frozen = True
            out.append(dict(
                name=(name, S),
                shape=tuple(rows.shape) == (el, p * S) + tuple(x.shape[1:]) and rows.dtype == x.dtype,
                rows=same_bits(rows, want["rows"]), pads=pad.pads_are_zero_bits(rows, plan.valid, S),
                slots=torch.equal(plan.slots, want["slots"]), kept=torch.equal(plan.kept, want["kept"]),
                valid=torch.equal(plan.valid, want["valid"]), dropped=torch.equal(plan.dropped, want["dropped"]),
                dtypes=plan.kept.dtype == plan.valid.dtype == plan.dropped.dtype == torch.int64
                and tuple(plan.kept.shape) == (E,) and tuple(plan.valid.shape) == (el, p),
                back=same_bits(back, want["back"]), out=same_bits(got, want["out"]),
                direct=same_bits(got, moe_ref.direct(x, want["cut_ids"], w, E)),
                plan=plan.source_capacity == S and plan.expert_counts == (p * S,) * el
                and plan.send_counts == plan.recv_counts == (el * S,) * p and plan.matrix == ((el * S,) * p,) * p
                and plan.num_rows == E * S and plan.capacity is None,
                unknown=plan.clipped is None and plan.demand_matrix is None and plan.expert_matrix is None,
                frozen=frozen,
                untouched=same_bits(x, want["x"]) and torch.equal(ids, want["ids"]) and same_bits(w, want["w"]),
                delta=delta, gathers=len(calls)))
    finally:
        sparse._count_matrix = gather
    return out


KEYS = ("shape", "rows", "pads", "slots", "kept", "valid", "dropped", "dtypes", "back", "out", "direct", "plan",
        "unknown", "frozen", "untouched")


@pytest.mark.parametrize("p", [2, 3])
def test_host_tensors_equal_the_definition_with_no_count_exchange(p):
    res, _, _ = run_ranks(p, _table_on_host, timeout=120)
    assert sorted(res) == list(range(p))
    for r, rows in res.items():
        assert [row["name"] for row in rows] == pad.TABLE
        for row in rows:
            for key in KEYS:
                assert row[key], (r, row["name"], key)
            assert row["delta"] == {"moe.dispatch": 1, "moe.combine": 1, "moe.dispatch.padded": 1}, (r, row)
            assert row["gathers"] == 0, (r, row["name"])


def _above_all_demand(comm):
    """A share no rank's demand reaches: the uncapped call's output exactly, and its rows block by block."""
    from mp4x.parallel import sparse
    r, p = comm.getRank(), comm.getSlaveNum()
    out = []
    for name in sorted(moe_ref.CASES):
        want = moe_ref.end_to_end(name, p)[r]
        E, el = want["E"], want["E"] // p
        rows0, plan0 = comm.dispatchTokens(want["x"], want["ids"], E)
        calls, gather = _counting(sparse)
        try:
            rows, plan = comm.dispatchTokens(want["x"], want["ids"], E, sourceCapacity=pad.NO_CUT)
            got = comm.combineTokens(pad.apply_experts(rows, r * el), plan, want["w"])
        finally:
            sparse._count_matrix = gather
        # the ragged rows are the padded blocks' valid rows, expert by expert and source by source
        pieces = [rows[e, i * pad.NO_CUT:i * pad.NO_CUT + int(plan.valid[e, i])] for e in range(el) for i in range(p)]
        out.append(same_bits(got, want["out"]) and same_bits(torch.cat(pieces), rows0)
                   and [int(v) for v in plan.valid.sum(1)] == list(plan0.expert_counts)
                   and plan.dropped.tolist() == [0, int(want["counts"][E]), 0] and not calls
                   and plan.kept.tolist() == list(plan0.expert_matrix[r]))
    return out


def test_a_share_above_all_demand_equals_the_uncapped_call():
    res, _, _ = run_ranks(2, _above_all_demand, timeout=120)
    assert res == {0: [True] * 4, 1: [True] * 4}


def _one_backward(comm, dtype):
    """combineTokensBackward along a padded plan nothing is cut from and along the ragged plan of the
    same ids: (g_weights equal, gradient rows equal block by block, the padded pad rows +0), as bits."""
    r, p = comm.getRank(), comm.getSlaveNum()
    T, K, E, S = 5, 2, 4, 10                 # S = T * K: no (rank, expert) demand reaches it
    el = E // p
    x = moe_ref.tokens(T, 8, dtype, 41 + r)
    g = moe_ref.tokens(T, 8, dtype, 51 + r)
    ids = ((torch.arange(T * K) * 3 + r) % E).view(T, K)
    ids[2, 1] = -1
    w = moe_ref.gate_weights(T, K, 7 + r)
    rows_r, plan_r = comm.dispatchTokens(x, ids, E)
    rows_p, plan_p = comm.dispatchTokens(x, ids, E, sourceCapacity=S)
    _, back_r = comm.combineTokens(moe_ref.apply_experts(rows_r, plan_r.expert_counts, r * el), plan_r, w,
                                   returnSlotRows=True)
    _, back_p = comm.combineTokens(pad.apply_experts(rows_p, r * el), plan_p, w, returnSlotRows=True)
    g_rows_r, g_w_r = comm.combineTokensBackward(g, plan_r, w, back_r)
    g_rows_p, g_w_p = comm.combineTokensBackward(g, plan_p, w, back_p)
    pieces = [g_rows_p[e, i * S:i * S + int(plan_p.valid[e, i])] for e in range(el) for i in range(p)]
    return (same_bits(g_w_p, g_w_r), same_bits(torch.cat(pieces), g_rows_r) and g_rows_r.shape[0] > 0,
            pad.pads_are_zero_bits(g_rows_p, plan_p.valid, S) and tuple(g_rows_p.shape) == (el, p * S, 8))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("p", [1, 2])
def test_the_two_layouts_give_one_combine_backward(p, dtype):
    res, _, _ = run_ranks(p, _one_backward, args=(dtype,), timeout=120)
    assert res == {r: (True, True, True) for r in range(p)}


def _one_rank_and_bad_ids(comm):
    """p = 1 (no exchange at all) and ids >= E: slot -1, counted, never raised."""
    r, p = comm.getRank(), comm.getSlaveNum()
    E, S = 2 * p, 2
    ids = torch.tensor([[0, E], [0, E + 5], [0, 1], [-1, 1], [1, 0], [E - 1, -3]])
    w = moe_ref.gate_weights(6, 2, 5)
    want = pad.from_inputs([(moe_ref.tokens(6, 4, torch.float32, 31 + i), ids, w, E) for i in range(p)], S)[r]
    x = want["x"]
    rows, plan = comm.dispatchTokens(x, ids, E, sourceCapacity=S)
    got = comm.combineTokens(pad.apply_experts(rows, r * 2), plan, w)
    return (same_bits(rows, want["rows"]), torch.equal(plan.slots, want["slots"]), plan.dropped.tolist(),
            plan.kept.tolist() == want["kept"].tolist(), same_bits(got, want["out"]), want["dropped"].tolist())


@pytest.mark.parametrize("p", [1, 2])
def test_ids_past_the_experts_are_dropped_and_counted(p):
    res, _, _ = run_ranks(p, _one_rank_and_bad_ids, timeout=120)
    for r in range(p):
        rows, slots, dropped, kept, out, want = res[r]
        assert rows and slots and kept and out, (r, res[r])
        # expert 0 four times against S = 2 (and expert 1 three or four times), two negative ids, two ids >= E
        assert dropped == want == [3 if p == 2 else 4, 2, 2], (r, dropped, want)


# ---------------------------------------------------------------- refusals, on every rank
def _refusals(comm):
    from mp4x import Mp4jException
    from mp4x.parallel import sparse
    r, p = comm.getRank(), comm.getSlaveNum()
    E = 2 * p
    x = moe_ref.tokens(6, 4, torch.float32, 9 + r)
    ids = ((torch.arange(12) + r) % E).view(6, 2)
    w = moe_ref.gate_weights(6, 2, 3)
    calls = {
        "S 0": dict(sourceCapacity=0), "S -1": dict(sourceCapacity=-1), "S bool": dict(sourceCapacity=True),
        "S float": dict(sourceCapacity=2.0), "S str": dict(sourceCapacity="2"),
        "S tensor": dict(sourceCapacity=torch.tensor(2)),
        "with capacity": dict(sourceCapacity=2, capacity=2),
        "with factor": dict(sourceCapacity=2, capacityFactor=1.0),
        "with a bad capacity": dict(sourceCapacity=2, capacity=0),
    }
    seen = {}
    gathers, gather = _counting(sparse)
    before = dict(comm.device.stats)
    try:
        for label, kw in calls.items():
            try:
                comm.dispatchTokens(x, ids, E, **kw)
                seen[label] = "no error"
            except Mp4jException as e:
                seen[label] = str(e)
    finally:
        sparse._count_matrix = gather
    no_work = comm.device.stats.get("moe.dispatch.padded", 0) == before.get("moe.dispatch.padded", 0)
    # the two layouts do not mix
    rows_p, plan_p = comm.dispatchTokens(x, ids, E, sourceCapacity=2)
    rows_r, plan_r = comm.dispatch_tokens(x, ids, E)
    mixed = {}
    for label, (rows, plan) in {"ragged rows, padded plan": (rows_r, plan_p), "padded rows, ragged plan": (rows_p, plan_r),
                                "padded rows of another share": (rows_p[:, :-1].contiguous(), plan_p)}.items():
        try:
            comm.combineTokens(rows, plan, w)
            mixed[label] = "no error"
        except Mp4jException as e:
            mixed[label] = str(e)
    # ... and the communicator still works
    got = comm.combine_tokens(rows_p, plan_p, w)
    cut = pad.cut_ids(ids, E, 2)
    want = moe_ref.ref_combine(pad.send_buffer(x, cut[1], 2, E, 2), cut[1], w, 6, 2)
    return seen, mixed, len(gathers), no_work, same_bits(got, want)


@pytest.mark.parametrize("p", [2, 3])
def test_every_refusal_raises_on_every_rank_before_any_work(p):
    res, code, errors = run_ranks(p, _refusals, timeout=120)
    assert sorted(res) == list(range(p)) and not errors and code == 0
    for r, (seen, mixed, gathers, no_work, works) in res.items():
        assert len(seen) == 9 and len(mixed) == 3
        for label, msg in seen.items():
            assert msg != "no error" and "sourceCapacity" in msg, (r, label, msg)
        for label, msg in mixed.items():
            assert msg != "no error" and "padded" in msg, (r, label, msg)
        assert gathers == 0 and no_work and works, r


# ---------------------------------------------------------------- the native refusals
def _lib():
    try:
        return native.hip()
    except Exception as e:   # noqa: BLE001
        pytest.skip(f"libmp4x_hip.so not loadable: {e}")


IDS, X, OUT, SLOTS, SCRATCH, SCALE, KEPT, DROPPED = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x70000, 0x80000, 0x90000


def _scatter_pad(lib, dtype=DType.F32, ids=IDS, i64=1, x=X, scale=None, n=519, K=3, rb=16, nb=8, cap=4, out=OUT,
                 slots=SLOTS, scratch=SCRATCH, sb=None):
    sb = lib.mp4x_moe_route_scratch_bytes(n, nb) if sb is None else sb
    return lib.mp4x_moe_route_scatter_pad(int(dtype), ids, i64, x, scale, n, K, rb, nb, cap, out, slots, scratch, sb,
                                          None)


@pytest.mark.parametrize("case,want", [
    (dict(cap=0), BADARG), (dict(cap=-1), BADARG), (dict(cap=(1 << 31) // 8 + 1), BADARG),
    # the buffer is written whole even by the empty call: checked before it
    (dict(n=0, out=None), BADARG), (dict(n=0, out=OUT + 8), BADARG), (dict(n=0, cap=0), BADARG),
    # ... and everything the unclipped entry refuses
    (dict(dtype=DType.F64), UNSUPPORTED), (dict(dtype=DType.I32), UNSUPPORTED), (dict(dtype=99), UNSUPPORTED),
    (dict(nb=0), BADARG), (dict(nb=2049), BADARG), (dict(n=-3), BADARG), (dict(K=0), BADARG), (dict(n=520), BADARG),
    (dict(rb=0), BADARG), (dict(rb=24), BADARG),
    (dict(ids=None), BADARG), (dict(ids=IDS + 4), BADARG), (dict(x=None), BADARG), (dict(x=X + 8), BADARG),
    (dict(out=None), BADARG), (dict(out=OUT + 4), BADARG), (dict(slots=None), BADARG), (dict(slots=SLOTS + 4), BADARG),
    (dict(scale=SCALE + 2), BADARG), (dict(scratch=None), BADARG), (dict(scratch=SCRATCH + 8), BADARG),
    (dict(sb=128), BADARG), (dict(n=(1 << 30) + 2, K=1), BADARG),
])
def test_route_scatter_pad_refuses_without_launching(case, want):
    assert _scatter_pad(_lib(), **case) == want


def _pad_counts(lib, n=519, nb=8, cap=4, el=4, el_pad=4, kept=KEPT, dropped=DROPPED, scratch=SCRATCH, sb=None):
    sb = lib.mp4x_moe_route_scratch_bytes(n, nb) if sb is None else sb
    return lib.mp4x_moe_pad_counts(n, nb, cap, el, el_pad, kept, dropped, scratch, sb, None)


@pytest.mark.parametrize("case", [
    dict(cap=0), dict(nb=0), dict(nb=2049), dict(n=-1), dict(n=1 << 31), dict(el=0), dict(el=3), dict(el_pad=3),
    dict(kept=None), dict(kept=KEPT + 4), dict(dropped=None), dict(dropped=DROPPED + 4), dict(scratch=None),
    dict(scratch=SCRATCH + 8), dict(sb=128), dict(n=0, kept=None), dict(n=0, cap=0),
])
def test_pad_counts_refuses_without_launching(case):
    assert _pad_counts(_lib(), **case) == BADARG


def _combine_rows(lib, dtype=DType.F32, rows=X, num_rows=32, slots=SLOTS, weights=None, T=6, K=2, width=4, out=OUT):
    return lib.mp4x_moe_combine_rows(int(dtype), rows, num_rows, slots, weights, T, K, width, out, None)


@pytest.mark.parametrize("case,want", [
    (dict(num_rows=0), BADARG), (dict(num_rows=-1), BADARG), (dict(dtype=DType.F64), UNSUPPORTED),
    (dict(T=-1), BADARG), (dict(K=0), BADARG), (dict(width=0), BADARG), (dict(width=3), BADARG),
    (dict(rows=None), BADARG), (dict(rows=X + 8), BADARG), (dict(out=None), BADARG), (dict(out=OUT + 4), BADARG),
    (dict(slots=None), BADARG), (dict(slots=SLOTS + 4), BADARG), (dict(weights=SCALE + 2), BADARG),
])
def test_combine_rows_refuses_without_launching(case, want):
    assert _combine_rows(_lib(), **case) == want


def test_the_empty_combine_returns_zero_without_a_launch():
    assert _combine_rows(_lib(), T=0, rows=None, out=None, slots=None) == 0
