"""dispatchTokens / combineTokens without a GPU: host tensors over the gloo all-to-all against the
contract (tests/moe_ref.py), the count-exchange and counter bookkeeping, every refusal on every
rank, one rank, and the native refusals of the K9 entry points on the real libmp4x_hip.so (fake
pointers: the checks are host-side and launch nothing)."""
import pytest

torch = pytest.importorskip("torch")

import moe_ref  # noqa: E402
from harness import run_ranks  # noqa: E402
from moe_ref import CASES, same_bits  # noqa: E402
from mp4x.operators import DType  # noqa: E402
from mp4x.ops import native  # noqa: E402

BADARG, UNSUPPORTED = 1001, 1002


# ---------------------------------------------------------------- the contract helper itself
@pytest.mark.parametrize("p", [1, 2, 3])
@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_end_to_end_equals_the_direct_formula(name, p):
    res = moe_ref.end_to_end(name, p)                        # asserts the properties and the formula
    for r, row in enumerate(res):
        assert sum(row["expert_counts"]) == row["rows"].shape[0]
        assert int((row["slots"] >= 0).sum()) == row["send"].shape[0]


def test_reference_fp8_shape():
    moe_ref.check_case_properties("D8", 2)


# ---------------------------------------------------------------- host tensors through the API
def _cases_on_host(comm):
    from mp4x.parallel import sparse
    r, p = comm.getRank(), comm.getSlaveNum()
    stats = comm.device.stats
    out = []
    for name in sorted(CASES):
        want = moe_ref.end_to_end(name, p)[r]
        gathers, gather = [], sparse._count_matrix
        sparse._count_matrix = lambda *a: gathers.append(1) or gather(*a)
        try:
            before = dict(stats)
            rows, plan = comm.dispatchTokens(want["x"].clone(), want["ids"].clone(), want["E"])
            after_dispatch = (len(gathers), stats.get("moe.dispatch", 0) - before.get("moe.dispatch", 0),
                              stats.get("moe.combine", 0) - before.get("moe.combine", 0))
            y = moe_ref.apply_experts(rows, plan.expert_counts, r * (want["E"] // p))
            before = dict(stats)
            got = comm.combine_tokens(y, plan, want["w"].clone())
            again, back = comm.combineTokens(y, plan, want["w"].clone(), returnSlotRows=True)
            after_combine = (len(gathers) - after_dispatch[0],
                             stats.get("moe.dispatch", 0) - before.get("moe.dispatch", 0),
                             stats.get("moe.combine", 0) - before.get("moe.combine", 0))
        finally:
            sparse._count_matrix = gather
        frozen = False
        try:
            plan.top_k = 7
        except AttributeError:
            frozen = True
        out.append(dict(
            name=name, rows=same_bits(rows, want["rows"]), counts=list(plan.expert_counts) == want["expert_counts"],
            slots=torch.equal(plan.slots, want["slots"]), out=same_bits(got, want["out"]),
            again=same_bits(again, want["out"]), back=same_bits(back, want["back"]),
            mat=[list(x) for x in plan.matrix] == want["mat"],
            meta=(plan.num_tokens, plan.top_k, plan.num_experts) == (want["x"].shape[0], want["ids"].shape[1], want["E"]),
            send=list(plan.send_counts) == want["mat"][r], recv=list(plan.recv_counts) == [m[r] for m in want["mat"]],
            after_dispatch=after_dispatch, after_combine=after_combine, frozen=frozen))
    return out


@pytest.mark.parametrize("p", [1, 2, 3])
def test_host_tensors_equal_the_reference(p):
    res, _, _ = run_ranks(p, _cases_on_host, timeout=120)
    assert sorted(res) == list(range(p))
    for r, rows in res.items():
        assert len(rows) == 4
        for row in rows:
            what = (r, row["name"])
            for key in ("rows", "counts", "slots", "out", "again", "back", "mat", "meta", "send", "recv", "frozen"):
                assert row[key], (what, key)
            # one count exchange per dispatch (none with one rank), never one per combine
            assert row["after_dispatch"] == (1 if p > 1 else 0, 1, 0), (what, row["after_dispatch"])
            assert row["after_combine"] == (0, 0, 2), (what, row["after_combine"])


def _one_d_ids_and_unit_weights(comm):
    r, p = comm.getRank(), comm.getSlaveNum()
    E = 2 * p
    x = moe_ref.tokens(9, 4, torch.float32, 77 + r)
    ids = (torch.arange(9) + r) % E
    rows, plan = comm.dispatch_tokens(x, ids.to(torch.int32), E)
    got = comm.combineTokens(rows, plan)
    return same_bits(got, x) and plan.top_k == 1


def test_ids_of_one_dimension_and_no_weights():
    res, _, _ = run_ranks(2, _one_d_ids_and_unit_weights, timeout=120)
    assert res == {0: True, 1: True}


# ---------------------------------------------------------------- refusals, on every rank
def _refusals(comm):
    from mp4x import Mp4jException
    r, p = comm.getRank(), comm.getSlaveNum()
    E = 2 * p
    x = moe_ref.tokens(6, 4, torch.float32, 9 + r)
    ids = ((torch.arange(12) + r) % E).view(6, 2)
    w = moe_ref.gate_weights(6, 2, 3)
    rows, plan = comm.dispatchTokens(x, ids, E)
    bad_id = ids.clone()
    if r == p - 1:
        bad_id[3, 1] = E                                     # one rank only: known everywhere from the counts

    calls = {
        "E % p": lambda: comm.dispatchTokens(x, ids, E + 1),
        "E > 2048": lambda: comm.dispatchTokens(x, ids, 2048 + p),
        "ids rows": lambda: comm.dispatchTokens(x, ids[:5], E),
        "ids dims": lambda: comm.dispatchTokens(x, ids.view(6, 2, 1), E),
        "ids dtype": lambda: comm.dispatchTokens(x, ids.to(torch.float32), E),
        "id >= E": lambda: comm.dispatchTokens(x, bad_id, E),
        "dtype": lambda: comm.dispatchTokens(x.to(torch.float64), ids, E),
        "int dtype": lambda: comm.dispatchTokens(x.to(torch.int32), ids, E),
        "not contiguous": lambda: comm.dispatchTokens(x.t().contiguous().t(), ids, E),
        "weights dtype": lambda: comm.combineTokens(rows, plan, w.to(torch.float64)),
        "weights shape": lambda: comm.combineTokens(rows, plan, w[:5]),
        "rows count": lambda: comm.combineTokens(torch.cat([rows, rows[:1]]), plan, w),
        "rows dtype": lambda: comm.combineTokens(rows.to(torch.bfloat16), plan, w),
        "plan": lambda: comm.combineTokens(rows, (1, 2), w),
    }
    seen = {}
    for label, call in calls.items():
        try:
            call()
            seen[label] = "no error"
        except Mp4jException as e:
            seen[label] = str(e)
    # ... and the communicator still works
    back = comm.combineTokens(rows, plan, w)
    want = moe_ref.ref_combine(moe_ref.ref_send(x, moe_ref.ref_route(ids, E)[2], 2), moe_ref.ref_route(ids, E)[1], w, 6, 2)
    return seen, same_bits(back, want)


@pytest.mark.parametrize("p", [2, 3])
def test_every_refusal_raises_on_every_rank_and_the_job_closes(p):
    res, code, errors = run_ranks(p, _refusals, timeout=120)
    assert sorted(res) == list(range(p)) and not errors and code == 0
    for r, (seen, works) in res.items():
        assert works, r
        assert len(seen) == 14
        for label, msg in seen.items():
            assert msg != "no error", (r, label)
        assert f"rank {p - 1}" in seen["id >= E"], (r, seen["id >= E"])


# ---------------------------------------------------------------- the native refusals
def _lib():
    try:
        return native.hip()
    except Exception as e:   # noqa: BLE001
        pytest.skip(f"libmp4x_hip.so not loadable: {e}")


IDS, X, OUT, SLOTS, SCRATCH, COUNTS, SCALE = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000


def _count(lib, ids=IDS, i64=1, n=519, nb=8, counts=COUNTS, scratch=SCRATCH, sb=None):
    sb = lib.mp4x_moe_route_scratch_bytes(n, nb) if sb is None else sb
    return lib.mp4x_moe_route_count(ids, i64, n, nb, counts, scratch, sb, None)


def _scatter(lib, dtype=DType.F32, ids=IDS, i64=1, x=X, scale=None, n=519, K=3, rb=16, nb=8, out=OUT, slots=SLOTS,
             scratch=SCRATCH, sb=None):
    sb = lib.mp4x_moe_route_scratch_bytes(n, nb) if sb is None else sb
    return lib.mp4x_moe_route_scatter(int(dtype), ids, i64, x, scale, n, K, rb, nb, out, slots, scratch, sb, None)


def _combine(lib, dtype=DType.F32, rows=X, slots=SLOTS, w=None, T=173, K=3, width=4, out=OUT):
    return lib.mp4x_moe_combine(int(dtype), rows, slots, w, T, K, width, out, None)


@pytest.mark.parametrize("case", [
    dict(nb=0), dict(nb=2049), dict(n=-1), dict(counts=None), dict(counts=COUNTS + 4), dict(ids=None),
    dict(ids=IDS + 4), dict(i64=0, ids=IDS + 2), dict(scratch=None), dict(scratch=SCRATCH + 16), dict(sb=64),
    dict(n=(1 << 30) + 1),
])
def test_route_count_refuses_without_launching(case):
    assert _count(_lib(), **case) == BADARG


@pytest.mark.parametrize("case,want", [
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
def test_route_scatter_refuses_without_launching(case, want):
    assert _scatter(_lib(), **case) == want


@pytest.mark.parametrize("case,want", [
    (dict(dtype=DType.F64), UNSUPPORTED), (dict(dtype=DType.I64), UNSUPPORTED), (dict(dtype=DType.I8), UNSUPPORTED),
    (dict(T=-1), BADARG), (dict(K=0), BADARG), (dict(width=0), BADARG), (dict(width=6), BADARG),
    (dict(dtype=DType.BF16, width=4), BADARG),                # 8 bytes per row
    (dict(rows=None), BADARG), (dict(rows=X + 8), BADARG), (dict(out=None), BADARG), (dict(out=OUT + 2), BADARG),
    (dict(slots=None), BADARG), (dict(slots=SLOTS + 4), BADARG), (dict(w=SCALE + 1), BADARG),
    (dict(T=1 << 30, K=2), BADARG),
])
def test_combine_refuses_without_launching(case, want):
    assert _combine(_lib(), **case) == want


def test_empty_calls_return_zero_without_a_launch():
    lib = _lib()
    assert _scatter(lib, n=0, ids=None, x=None, out=None, slots=None, scratch=None, sb=0) == 0
    assert _combine(lib, T=0, rows=None, slots=None, out=None) == 0
    # (the empty count zeroes counts[nb + 2] with a memset: it needs a device, tests/test_moe_kernels_gpu.py)
