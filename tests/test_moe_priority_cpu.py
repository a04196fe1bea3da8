"""Drop by gate weight without a GPU: ``priority_mask_torch`` against the plain-Python definition
(tests/moe_priority_ref.py) on the select's case table, the two consequences of the definition (a
constant priority is the position policy; expert e keeps min(cnt, limit)), and ``dispatchTokens(...,
priority=)`` on host tensors over gloo: the padded and the capped ragged call are, bit for bit, the
plain call on the reference-masked ids, ``dropped`` keeps its meaning, and the refusals."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import moe_priority_ref as ref  # noqa: E402
import moe_ref  # noqa: E402
from harness import run_ranks  # noqa: E402
from moe_ref import same_bits  # noqa: E402
from mp4x.parallel.moe import capacity_quota, priority_mask_torch  # noqa: E402


def _check(ids, prio, nb, limit):
    want, want_masked = ref.mask_tensors(ids, prio, nb, limit)
    got, masked = priority_mask_torch(ids, prio, nb, limit)
    assert got.dtype == ids.dtype and got.shape == ids.shape
    assert torch.equal(got, want)
    assert masked.dtype == torch.int64 and masked.tolist() == [want_masked]
    return got


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("n,nb", ref.SHAPES)
def test_the_torch_form_equals_the_definition(n, nb, kind):
    ids = ref.ids_for(n, nb, 17 * n + nb)
    prio = ref.priorities(kind, n, n + nb)
    for idt in (torch.int64, torch.int32):
        _check(ids.to(idt), prio, nb, ref.limit_vector(ids, nb, nb))
        _check(ids.to(idt), prio, nb, 1)


def test_all_assignments_to_one_expert():
    ids = torch.full((600,), 2, dtype=torch.int64)
    for kind in ref.KINDS:
        got = _check(ids, ref.priorities(kind, 600, 5), 3, 5)
        assert int((got == 2).sum()) == 5


def test_strays_pass_through_and_a_2d_shape_is_kept():
    ids = torch.tensor([[0, -1], [5, 0], [0, -7], [9, 0]])
    got = _check(ids, torch.tensor([[.1, .9], [.9, .3], [.2, .9], [.9, .4]]), 5, 2)
    assert got.tolist() == [[-1, -1], [5, 0], [-1, -7], [9, 0]]


@pytest.mark.parametrize("n,nb", ref.SHAPES)
def test_a_constant_priority_is_the_position_policy(n, nb):
    ids = ref.ids_for(n, nb, 3 * n + nb)
    for limit in (ref.limit_vector(ids, nb, 1), 2):
        got, _ = priority_mask_torch(ids, ref.priorities("constant", n, 0), nb, limit)
        lim = limit if isinstance(limit, int) else limit.tolist()
        assert got.tolist() == ref.position_mask(ids.tolist(), nb, lim)


@pytest.mark.parametrize("kind", ref.KINDS)
def test_every_expert_keeps_min_of_count_and_limit(kind):
    n, nb = 600, 7
    ids = ref.ids_for(n, nb, 77)
    lim = ref.limit_vector(ids, nb, 2)
    got, masked = priority_mask_torch(ids, ref.priorities(kind, n, 9), nb, lim)
    placed = (ids >= 0) & (ids < nb)
    cnt = torch.bincount(ids[placed], minlength=nb)
    kept = torch.bincount(got[(got >= 0) & (got < nb)], minlength=nb)
    assert torch.equal(kept, torch.minimum(cnt, lim))
    assert int(masked) == int((cnt - kept).sum())
    assert torch.equal(got[~placed], ids[~placed])


# ---------------------------------------------------------------- dispatch on host tensors
def _dispatch_on_host(comm, name, padded):
    r, p = comm.getRank(), comm.getSlaveNum()
    T, K, el, width, S, C = ref.DISPATCH[name]
    per_rank = [ref.dispatch_case(name, i, p) for i in range(p)]
    x, ids, w, E = per_rank[r]
    counts = [np.bincount(i.reshape(-1).numpy()[i.reshape(-1).numpy() >= 0], minlength=E) for _, i, _, _ in per_rank]
    if padded:
        limit = S
        kw, plain_kw = dict(sourceCapacity=S), dict(sourceCapacity=S)
    else:
        limit = list(capacity_quota([c.tolist() for c in counts], C)[r])
        kw, plain_kw = dict(capacity=C), {}
    ids_m, masked = ref.mask_tensors(ids, w, E, limit)
    rows, plan = comm.dispatchTokens(x, ids, E, priority=w, **kw)
    rows0, plan0 = comm.dispatchTokens(x, ids_m, E, **plain_kw)
    first = r * el
    if padded:
        import moe_padded_ref as pad
        y, y0 = pad.apply_experts(rows, first), pad.apply_experts(rows0, first)
    else:
        y = moe_ref.apply_experts(rows, plan.expert_counts, first)
        y0 = moe_ref.apply_experts(rows0, plan0.expert_counts, first)
    out, back = comm.combineTokens(y, plan, w, returnSlotRows=True)
    out0, back0 = comm.combineTokens(y0, plan0, w, returnSlotRows=True)
    g = moe_ref.tokens(T, width, torch.float32, 77 + r)
    g_rows, g_w = comm.combineTokensBackward(g, plan, w, back)
    g_rows0, g_w0 = comm.combineTokensBackward(g, plan0, w, back0)
    res = dict(rows=same_bits(rows, rows0), slots=torch.equal(plan.slots, plan0.slots), out=same_bits(out, out0),
               back=same_bits(back, back0), g_rows=same_bits(g_rows, g_rows0), g_w=same_bits(g_w, g_w0),
               direct=same_bits(out, moe_ref.direct(x, ids_m, w, E)), cut=masked,
               differs=ids_m.reshape(-1).tolist() != ref.position_mask(ids.reshape(-1).tolist(), E, limit),
               counts=plan.expert_counts == plan0.expert_counts and plan.send_counts == plan0.send_counts
               and plan.recv_counts == plan0.recv_counts and plan.matrix == plan0.matrix)
    neg = int((ids < 0).sum())
    if padded:
        res.update(kept=torch.equal(plan.kept, plan0.kept), valid=torch.equal(plan.valid, plan0.valid),
                   dropped=plan.dropped.tolist() == [masked, neg, 0] and plan0.dropped.tolist() == [0, neg + masked, 0]
                   and plan.dropped.dtype == torch.int64)
    else:
        _, pos = comm.dispatchTokens(x, ids, E, **kw)          # every host-side field is the position call's
        res.update(host=plan.expert_matrix == pos.expert_matrix and plan.demand_matrix == pos.demand_matrix
                   and plan.clipped == pos.clipped == masked and plan.matrix == pos.matrix and plan.capacity == C
                   and plan.expert_counts == pos.expert_counts and plan.send_counts == pos.send_counts
                   and plan.recv_counts == pos.recv_counts and plan._clip is None)
    return res


@pytest.mark.parametrize("padded", [True, False], ids=["padded", "capacity"])
@pytest.mark.parametrize("name", sorted(ref.DISPATCH))
@pytest.mark.parametrize("p", [2, 3])
def test_a_priority_dispatch_is_the_plain_call_on_the_masked_ids(p, name, padded):
    res, _, _ = run_ranks(p, _dispatch_on_host, args=(name, padded), timeout=120)
    assert sorted(res) == list(range(p))
    for r, row in res.items():
        for key, val in row.items():
            if key not in ("cut", "differs"):
                assert val is True, (r, key, row)
    assert sum(row["cut"] for row in res.values()) > 0          # something was dropped ...
    assert any(row["differs"] for row in res.values())          # ... and not what the position policy drops


# ---------------------------------------------------------------- the native refusals (fake pointers: nothing launches)
BADARG = 1001
IDS, PRIO, OUT, ROUTE, SCRATCH, MASKED, LIMIT = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000


def _lib():
    from mp4x.ops import native
    try:
        return native.hip()
    except Exception as e:   # noqa: BLE001
        pytest.skip(f"libmp4x_hip.so not loadable: {e}")


def _mask(lib, ids=IDS, i64=1, prio=PRIO, n=519, nb=8, limit=3, vec=None, route=ROUTE, rb=None, out=OUT, masked=MASKED,
          scratch=SCRATCH, sb=None):
    rb = lib.mp4x_moe_route_scratch_bytes(n, nb) if rb is None else rb
    sb = lib.mp4x_moe_priority_scratch_bytes(n, nb) if sb is None else sb
    return lib.mp4x_moe_priority_mask(ids, i64, prio, n, nb, limit, vec, route, rb, out, masked, scratch, sb, None)


@pytest.mark.parametrize("case", [
    dict(nb=0), dict(nb=2049), dict(n=-1), dict(n=(1 << 30) + 2), dict(limit=-1), dict(vec=LIMIT + 4),
    dict(ids=None), dict(ids=IDS + 4), dict(i64=0, ids=IDS + 2), dict(prio=None), dict(prio=PRIO + 2),
    dict(out=None), dict(out=OUT + 4), dict(out=IDS), dict(masked=None), dict(masked=MASKED + 4),
    dict(route=None), dict(route=ROUTE + 8), dict(rb=128), dict(scratch=None), dict(scratch=SCRATCH + 8), dict(sb=128),
    dict(n=0, masked=None),
])
def test_the_entry_refuses_without_launching(case):
    assert _mask(_lib(), **case) == BADARG


def test_scratch_bytes_of_refused_arguments_is_zero():
    lib = _lib()
    assert lib.mp4x_moe_priority_scratch_bytes(519, 8) >= 519 * 8 + 8 * 16 + 3 * 8
    for n, nb in ((-1, 8), (1 << 30, 8), (519, 0), (519, 2049)):
        assert lib.mp4x_moe_priority_scratch_bytes(n, nb) == 0


def _refusals(comm):
    from mp4x import Mp4jException
    r, p = comm.getRank(), comm.getSlaveNum()
    E = 2 * p
    x = moe_ref.tokens(6, 4, torch.float32, 9 + r)
    ids = ((torch.arange(12) + r) % E).view(6, 2)
    w = moe_ref.gate_weights(6, 2, 3)
    calls = {
        "no capacity": dict(priority=w),
        "float64": dict(priority=w.double(), sourceCapacity=2),
        "shape": dict(priority=w[:, :1].contiguous(), sourceCapacity=2),
        "flat": dict(priority=w.reshape(-1), capacity=2),
        "strided": dict(priority=w.t().contiguous().t(), capacityFactor=1.0),
        "no tensor": dict(priority=[[0.5, 0.5]] * 6, sourceCapacity=2),
    }
    seen = {}
    for label, kw in calls.items():
        try:
            comm.dispatchTokens(x, ids, E, **kw)
            seen[label] = "no error"
        except Mp4jException as e:
            seen[label] = str(e)
    # ... and the communicator still works; a 1-D call takes a 1-D priority
    rows, plan = comm.dispatch_tokens(x, ids[:, 0].contiguous(), E, sourceCapacity=1, priority=w[:, 0].contiguous())
    want, _ = ref.mask_tensors(ids[:, 0], w[:, 0], E, 1)
    _, plan0 = comm.dispatchTokens(x, want, E, sourceCapacity=1)
    return seen, torch.equal(plan.slots, plan0.slots)


def test_the_refusals_raise_on_every_rank():
    res, code, errors = run_ranks(2, _refusals, timeout=120)
    assert sorted(res) == [0, 1] and not errors and code == 0
    for r, (seen, works) in res.items():
        assert len(seen) == 6 and works
        for label, msg in seen.items():
            assert msg != "no error" and "priority" in msg, (r, label, msg)
