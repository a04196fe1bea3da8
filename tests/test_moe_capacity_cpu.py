"""The expert capacity of dispatchTokens without a GPU: the quota against the first-come reference
(tests/moe_capacity_ref.py), host tensors over gloo against the reference and against the uncapped
call on the clipped ids, the plan's new fields, the count-exchange bookkeeping, capacityFactor, every
refusal on every rank, and the native refusals of mp4x_moe_route_scatter_clip on the real
libmp4x_hip.so (fake pointers: the checks are host-side and launch nothing)."""
import math

import pytest

torch = pytest.importorskip("torch")

import moe_capacity_ref as cap  # noqa: E402
import moe_ref  # noqa: E402
from harness import run_ranks  # noqa: E402
from moe_ref import same_bits  # noqa: E402
from mp4x.operators import DType  # noqa: E402
from mp4x.ops import native  # noqa: E402

BADARG, UNSUPPORTED = 1001, 1002


# ---------------------------------------------------------------- the quota
@pytest.mark.parametrize("p", [1, 2, 3])
@pytest.mark.parametrize("name,C", cap.EVERY)
def test_quota_equals_the_first_come_walk(name, C, p):
    from mp4x.parallel.moe import capacity_quota
    res = cap.end_to_end(name, p, C)                             # asserts the table's kept totals
    keep = capacity_quota(res[0]["demand"], C)
    assert [list(row) for row in keep] == res[0]["keep"]
    assert all(max(row) <= C for row in keep)
    for e in range(res[0]["E"]):
        assert sum(row[e] for row in keep) == min(C, sum(row[e] for row in res[0]["demand"]))


def test_quota_on_a_hand_made_matrix():
    from mp4x.parallel.moe import capacity_quota
    assert capacity_quota([[5, 0, 3], [4, 2, 9], [1, 1, 1]], 6) == ((5, 0, 3), (1, 2, 3), (0, 1, 0))
    assert capacity_quota([[5, 0, 3]], 1) == ((1, 0, 1),)
    assert capacity_quota([[5, 0, 3], [4, 2, 9]], 100) == ((5, 0, 3), (4, 2, 9))


def test_a_plan_built_without_the_new_fields_is_still_valid():
    from mp4x.parallel.moe import TokenPlan
    plan = TokenPlan(num_tokens=1, top_k=1, num_experts=2, expert_counts=(1,), send_counts=(1,), recv_counts=(1,),
                     slots=torch.zeros(1, dtype=torch.int64), matrix=((1,),), expert_matrix=((1, 0),), row_shape=(4,),
                     dtype=torch.float32, rank=0, _route=None)
    assert plan.capacity is None and plan.clipped == 0 and plan.demand_matrix == ((1, 0),)
    for name in ("capacity", "clipped", "demand_matrix"):
        with pytest.raises(AttributeError):
            setattr(plan, name, 3)


# ---------------------------------------------------------------- host tensors through the API
def _one(comm, want, ids, r, p, **kw):
    from mp4x.parallel import sparse
    stats = comm.device.stats
    gathers, gather = [], sparse._count_matrix
    sparse._count_matrix = lambda *a: gathers.append(1) or gather(*a)
    try:
        before = dict(stats)
        rows, plan = comm.dispatchTokens(want["x"].clone(), ids.clone(), want["E"], **kw)
        after_dispatch = (len(gathers), stats.get("moe.dispatch", 0) - before.get("moe.dispatch", 0),
                          stats.get("moe.combine", 0) - before.get("moe.combine", 0))
        y = moe_ref.apply_experts(rows, plan.expert_counts, r * (want["E"] // p))
        before = dict(stats)
        got = comm.combineTokens(y, plan, want["w"].clone())
        after_combine = (len(gathers) - after_dispatch[0], stats.get("moe.dispatch", 0) - before.get("moe.dispatch", 0),
                         stats.get("moe.combine", 0) - before.get("moe.combine", 0))
    finally:
        sparse._count_matrix = gather
    return rows, plan, got, after_dispatch, after_combine


def _cases_on_host(comm):
    r, p = comm.getRank(), comm.getSlaveNum()
    out = []
    for name, C in cap.EVERY:
        want = cap.end_to_end(name, p, C)[r]
        rows, plan, got, after_dispatch, after_combine = _one(comm, want, want["ids"], r, p, capacity=C)
        rows2, plan2, got2, _, _ = _one(comm, want, want["clipped_ids"], r, p)
        as_lists = lambda m: [list(row) for row in m]                                    # noqa: E731
        frozen = False
        try:
            plan.clipped = 0
        except AttributeError:
            frozen = True
        out.append(dict(
            name=(name, C),
            # against the reference
            rows=same_bits(rows, want["rows"]), slots=torch.equal(plan.slots, want["slots"]),
            counts=list(plan.expert_counts) == want["expert_counts"], mat=as_lists(plan.matrix) == want["mat"],
            emat=as_lists(plan.expert_matrix) == want["emat"], out=same_bits(got, want["out"]),
            send=list(plan.send_counts) == want["mat"][r], recv=list(plan.recv_counts) == [m[r] for m in want["mat"]],
            # against the uncapped call on the clipped ids
            rows2=same_bits(rows, rows2), slots2=torch.equal(plan.slots, plan2.slots),
            counts2=plan.expert_counts == plan2.expert_counts, mat2=plan.matrix == plan2.matrix,
            emat2=plan.expert_matrix == plan2.expert_matrix, out2=same_bits(got, got2),
            sr2=(plan.send_counts, plan.recv_counts) == (plan2.send_counts, plan2.recv_counts),
            # the plan
            demand=as_lists(plan.demand_matrix) == want["demand"], clipped=plan.clipped == want["clipped"],
            capacity=plan.capacity == C and type(plan.capacity) is int,
            plain=plan2.capacity is None and plan2.clipped == 0 and plan2.demand_matrix == plan2.expert_matrix,
            kept=int((plan.slots >= 0).sum()) == sum(want["keep"][r]), frozen=frozen,
            after_dispatch=after_dispatch, after_combine=after_combine))
    return out


KEYS = ("rows", "slots", "counts", "mat", "emat", "out", "send", "recv", "rows2", "slots2", "counts2", "mat2", "emat2",
        "out2", "sr2", "demand", "clipped", "capacity", "plain", "kept", "frozen")


@pytest.mark.parametrize("p", [1, 2, 3])
def test_host_tensors_equal_the_reference_and_the_uncapped_call_on_the_clipped_ids(p):
    res, _, _ = run_ranks(p, _cases_on_host, timeout=120)
    assert sorted(res) == list(range(p))
    for r, rows in res.items():
        assert [row["name"] for row in rows] == cap.EVERY
        for row in rows:
            what = (r, row["name"])
            for key in KEYS:
                assert row[key], (what, key)
            # one count exchange per dispatch (none with one rank), never one per combine
            assert row["after_dispatch"] == (1 if p > 1 else 0, 1, 0), (what, row["after_dispatch"])
            assert row["after_combine"] == (0, 0, 1), (what, row["after_combine"])


def _above_all_demand(comm):
    """A capacity nothing reaches: the uncapped call's result exactly (on the unclipped ids)."""
    r, p = comm.getRank(), comm.getSlaveNum()
    out = []
    for name in sorted(moe_ref.CASES):
        want = moe_ref.end_to_end(name, p)[r]
        rows, plan = comm.dispatchTokens(want["x"], want["ids"], want["E"])
        rows2, plan2 = comm.dispatchTokens(want["x"], want["ids"], want["E"], capacity=cap.NO_CLIP)
        y = moe_ref.apply_experts(rows, plan.expert_counts, r * (want["E"] // p))
        out.append(same_bits(rows, rows2) and same_bits(rows2, want["rows"]) and torch.equal(plan.slots, plan2.slots)
                   and plan.expert_counts == plan2.expert_counts and plan.matrix == plan2.matrix
                   and plan.expert_matrix == plan2.expert_matrix == plan2.demand_matrix and plan2.clipped == 0
                   and plan2.capacity == cap.NO_CLIP
                   and same_bits(comm.combineTokens(y, plan2, want["w"]), want["out"]))
    return out


def test_a_capacity_above_all_demand_changes_nothing():
    res, _, _ = run_ranks(2, _above_all_demand, timeout=120)
    assert res == {0: [True] * 4, 1: [True] * 4}


# ---------------------------------------------------------------- capacityFactor
def _factor(comm):
    r, p = comm.getRank(), comm.getSlaveNum()
    out = {}
    # case A: N = 519 + 0 assignments (47 of them negative), E = 8: ceil(64.875) = 65, not 472 / 8 = 59
    want = cap.end_to_end("A", p, 65)[r]
    rows, plan = comm.dispatchTokens(want["x"], want["ids"], want["E"], capacityFactor=1.0)
    out["A"] = (plan.capacity, same_bits(rows, want["rows"]), torch.equal(plan.slots, want["slots"]), plan.clipped,
                want["clipped"])
    # case B: N = 20, E = 2: ceil(0.33 * 10) = 4
    want = cap.end_to_end("B", p, 4)[r]
    rows, plan = comm.dispatch_tokens(want["x"], want["ids"], want["E"], capacityFactor=0.33)
    out["B"] = (plan.capacity, same_bits(rows, want["rows"]), torch.equal(plan.slots, want["slots"]), plan.clipped,
                want["clipped"])
    # an int factor is a number too
    _, plan = comm.dispatchTokens(want["x"], want["ids"], want["E"], capacityFactor=1)
    out["int"] = plan.capacity
    # nobody has a token: N = 0, ceil(0) = 0, C = max(1, 0)
    x = torch.empty(0, 4)
    rows, plan = comm.dispatchTokens(x, torch.empty(0, 2, dtype=torch.int64), 2 * p, capacityFactor=0.5)
    out["empty"] = (plan.capacity, rows.shape[0], plan.clipped)
    # one assignment in the whole job against 4 experts: ceil(0.5 / 4) = 1 = max(1, .) either way
    ids = torch.full((1, 1), 3) if r == 0 else torch.empty(0, 1, dtype=torch.int64)
    rows, plan = comm.dispatchTokens(torch.ones(ids.shape[0], 4), ids, 2 * p, capacityFactor=0.5)
    out["one"] = (plan.capacity, sum(plan.send_counts), plan.clipped)
    return out


def test_capacity_factor_resolves_to_the_documented_capacity():
    res, _, _ = run_ranks(2, _factor, timeout=120)
    assert math.ceil(1.0 * 519 / 8) == 65 and math.ceil(0.33 * 20 / 2) == 4
    for r in (0, 1):
        cA, rowsA, slotsA, clippedA, wantA = res[r]["A"]
        assert cA == 65 and rowsA and slotsA and clippedA == wantA, (r, res[r]["A"])
        cB, rowsB, slotsB, clippedB, wantB = res[r]["B"]
        assert cB == 4 and rowsB and slotsB and clippedB == wantB, (r, res[r]["B"])
        assert res[r]["int"] == 10
        assert res[r]["empty"] == (1, 0, 0), (r, res[r]["empty"])
        assert res[r]["one"] == (1, 1 if r == 0 else 0, 0), (r, res[r]["one"])
    assert res[0]["A"][3] > 0 and res[1]["B"][3] > 0             # ... and both of them clip


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
        "both": dict(capacity=2, capacityFactor=1.0),
        "capacity 0": dict(capacity=0), "capacity -1": dict(capacity=-1), "capacity bool": dict(capacity=True),
        "capacity float": dict(capacity=2.0), "capacity str": dict(capacity="2"),
        "capacity tensor": dict(capacity=torch.tensor(2)),
        "factor 0": dict(capacityFactor=0.0), "factor -1": dict(capacityFactor=-1.0),
        "factor inf": dict(capacityFactor=float("inf")), "factor nan": dict(capacityFactor=float("nan")),
        "factor bool": dict(capacityFactor=True), "factor str": dict(capacityFactor="1.0"),
    }
    seen = {}
    gathers, gather = [], sparse._count_matrix
    sparse._count_matrix = lambda *a: gathers.append(1) or gather(*a)
    try:
        for label, kw in calls.items():
            try:
                comm.dispatchTokens(x, ids, E, **kw)
                seen[label] = "no error"
            except Mp4jException as e:
                seen[label] = str(e)
    finally:
        sparse._count_matrix = gather
    # ... before the count exchange, and the communicator still works
    rows, plan = comm.dispatchTokens(x, ids, E, capacity=2)
    back = comm.combineTokens(rows, plan, w)
    cids, _, _ = cap.clip_ids([((torch.arange(12) + i) % E).view(6, 2) for i in range(p)], E, 2)
    route = moe_ref.ref_route(cids[r], E)
    want = moe_ref.ref_combine(moe_ref.ref_send(x, route[2], 2), route[1], w, 6, 2)
    return seen, len(gathers), same_bits(back, want)


@pytest.mark.parametrize("p", [2, 3])
def test_every_refusal_raises_on_every_rank_before_the_count_exchange(p):
    res, code, errors = run_ranks(p, _refusals, timeout=120)
    assert sorted(res) == list(range(p)) and not errors and code == 0
    for r, (seen, gathers, works) in res.items():
        assert len(seen) == 13
        for label, msg in seen.items():
            assert msg != "no error", (r, label)
            assert ("capacityFactor" if label.startswith("factor") else "capacity") in msg, (r, label, msg)
        assert gathers == 0, r
        assert works, r


# ---------------------------------------------------------------- the native refusals
def _lib():
    try:
        return native.hip()
    except Exception as e:   # noqa: BLE001
        pytest.skip(f"libmp4x_hip.so not loadable: {e}")


IDS, X, OUT, SLOTS, SCRATCH, SCALE, CLIP = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x70000, 0x80000


def _scatter_clip(lib, dtype=DType.F32, ids=IDS, i64=1, x=X, scale=None, n=519, K=3, rb=16, nb=8, out=OUT, slots=SLOTS,
                  clip=CLIP, scratch=SCRATCH, sb=None):
    sb = lib.mp4x_moe_route_scratch_bytes(n, nb) if sb is None else sb
    return lib.mp4x_moe_route_scatter_clip(int(dtype), ids, i64, x, scale, n, K, rb, nb, out, slots, clip, scratch, sb,
                                           None)


@pytest.mark.parametrize("case,want", [
    (dict(clip=None), BADARG), (dict(clip=CLIP + 4), BADARG), (dict(clip=CLIP + 1), BADARG),
    (dict(clip=None, n=0), BADARG),                           # the table is checked before the empty call returns
    # ... and everything the unclipped entry refuses
    (dict(dtype=DType.F64), UNSUPPORTED), (dict(dtype=DType.I32), UNSUPPORTED), (dict(dtype=DType.U8), UNSUPPORTED),
    (dict(dtype=99), UNSUPPORTED),
    (dict(nb=0), BADARG), (dict(nb=2049), BADARG), (dict(n=-3), BADARG), (dict(K=0), BADARG),
    (dict(n=520), BADARG),                                    # n is not T * K
    (dict(rb=0), BADARG), (dict(rb=24), BADARG),              # rows are whole 16-byte vectors
    (dict(ids=None), BADARG), (dict(ids=IDS + 4), BADARG), (dict(x=None), BADARG), (dict(x=X + 8), BADARG),
    (dict(out=None), BADARG), (dict(out=OUT + 4), BADARG), (dict(slots=None), BADARG), (dict(slots=SLOTS + 4), BADARG),
    (dict(scale=SCALE + 2), BADARG), (dict(scratch=None), BADARG), (dict(scratch=SCRATCH + 8), BADARG),
    (dict(sb=128), BADARG), (dict(n=(1 << 30) + 2, K=1), BADARG),
])
def test_route_scatter_clip_refuses_without_launching(case, want):
    assert _scatter_clip(_lib(), **case) == want


def test_the_empty_clipped_call_returns_zero_without_a_launch():
    assert _scatter_clip(_lib(), n=0, ids=None, x=None, out=None, slots=None, scratch=None, sb=0) == 0
