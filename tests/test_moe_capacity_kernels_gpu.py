"""The clipped K9 route scatter (csrc/kernels/moe.hip, ``moe_route_scatter(clip=)``), one process,
against the first-come reference of tests/moe_capacity_ref.py: ``slots`` exactly and the routed rows,
their ``row_scale`` form and the combine over the clipped slots bit for bit.  The quotas are given
directly.  ``out_rows`` carries guard rows past the kept total, pre-filled with a sentinel that must
survive; every launch runs twice and must give the same bits."""
import pytest

torch = pytest.importorskip("torch")

import moe_capacity_ref as cap  # noqa: E402
import moe_ref  # noqa: E402
from moe_ref import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD, SENTINEL = 3, 1024.0             # no token value (|x| <= 8) times a gate weight (< 1) reaches it


def _clip_table(keep):
    base, tot = [], 0
    for k in keep:
        base.append(tot)
        tot += k
    return torch.tensor(list(keep) + base, dtype=torch.int64, device=DEV), tot


def _run(x, ids, w, E, keep, scaled):
    """(slots, kept rows, guard rows, combine of the kept rows) of the clipped scatter."""
    from mp4x.ops import device_ops as ops
    T, K = ids.shape
    xd, idd, wd = x.to(DEV), ids.to(DEV), w.to(DEV)
    rc = ops.moe_route_count(idd.reshape(-1), E)
    clip, kept = _clip_table(keep)
    out = torch.full((kept + GUARD,) + tuple(x.shape[1:]), SENTINEL, dtype=x.dtype, device=DEV)
    slots = ops.moe_route_scatter(rc, xd, K, out, row_scale=wd.reshape(-1) if scaled else None, placed=kept, clip=clip)
    comb = ops.moe_combine(out[:kept], slots, None if scaled else wd, T, K, max_slot=kept - 1)
    torch.cuda.synchronize()
    return slots.cpu(), out[:kept].cpu(), out[kept:].cpu(), comb.cpu(), rc.counts.cpu()


def _expect(x, ids, w, E, keep, scaled):
    T, K = ids.shape
    (cid,), (kept,), _ = cap.clip_ids([ids], E, keep)
    _, slots, order = moe_ref.ref_route(cid, E)
    send = moe_ref.ref_send(x, order, K, w if scaled else None)
    return slots, send, moe_ref.ref_combine(send, slots, None if scaled else w, T, K), kept


def _check(x, ids, w, E, keep, what):
    for scaled in (False, True):
        slots, send, comb, kept = _expect(x, ids, w, E, keep, scaled)
        got = _run(x, ids, w, E, keep, scaled)
        again = _run(x, ids, w, E, keep, scaled)
        assert int((slots >= 0).sum()) == sum(kept) == got[1].shape[0], (what, scaled, "kept")
        assert torch.equal(got[0], slots), (what, scaled, "slots")
        assert same_bits(got[1], send), (what, scaled, "rows")
        assert bool((got[2] == SENTINEL).all()) and got[2].shape[0] == GUARD, (what, scaled, "guard rows")
        assert same_bits(got[3], comb), (what, scaled, "combine")
        assert torch.equal(got[0], again[0]) and same_bits(got[1], again[1]) and same_bits(got[3], again[3]), \
            (what, scaled, "run to run")
        # the count half knows nothing of the capacity
        assert torch.equal(got[4], moe_ref.ref_route(ids, E)[0]), (what, scaled, "counts")


@pytest.mark.parametrize("p", [2, 3])
@pytest.mark.parametrize("name,C", cap.EVERY)
def test_every_case_rank_0(name, C, p):
    want = cap.end_to_end(name, p, C)[0]
    x, ids, w, E, keep = want["x"], want["ids"], want["w"], want["E"], want["keep"][0]
    _check(x, ids, w, E, keep, (name, C, p))
    other = torch.int32 if ids.dtype == torch.int64 else torch.int64        # both id dtypes
    _check(x, ids.to(other), w, E, keep, (name, C, p, other))


@pytest.mark.parametrize("name,C,p,r", [("A", 40, 3, 2), ("B", 3, 3, 1), ("C", 6, 2, 1), ("C", 6, 3, 1), ("D", 300, 2, 1),
                                        ("D", 518, 2, 1)])
def test_the_partial_quotas_of_the_later_ranks(name, C, p, r):
    """What only a later rank sees: quotas that earlier ranks' demand has eaten into."""
    want = cap.end_to_end(name, p, C)[r]
    keep = want["keep"][r]
    assert 0 < sum(keep) < sum(want["demand"][r])
    _check(want["x"], want["ids"], want["w"], want["E"], keep, (name, C, p, r))


def _cuts(ids, E):
    """Quotas for T = 150, K = 2, E = 5: expert 0 cut at 0 (it has demand: the later bases shift),
    expert 1 cut exactly at the tile boundary (what it has among the first 256 assignments), expert
    2 cut inside a wave, expert 3 uncut, expert 4 cut after its first row."""
    flat = ids.reshape(-1)
    where = [(flat == e).nonzero().view(-1).tolist() for e in range(E)]
    demand = [len(ix) for ix in where]
    at_tile = sum(1 for a in where[1] if a < 256)
    assert 0 < at_tile < demand[1]
    mid = next(j for j in range(5, demand[2]) if where[2][j - 1] // 64 == where[2][j] // 64 and where[2][j] % 64)
    assert demand[0] > 0 and demand[3] > 0 and demand[4] > 1
    return [0, at_tile, mid, demand[3], 1], demand


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("vecs", [1, 3, 24, 65])      # 24 and 65: tiles split over 3 and 8 blocks
def test_dtypes_and_row_widths(dtype, vecs):
    dt = getattr(torch, dtype)
    width = vecs * 16 // torch.empty(0, dtype=dt).element_size()
    T, K, E = 150, 2, 5                                                      # n = 300: two tiles
    x = moe_ref.tokens(T, width, dt, 31 + vecs)
    w = moe_ref.gate_weights(T, K, 32 + vecs)
    g = torch.Generator().manual_seed(33 + vecs)
    ids = torch.randint(-1, E, (T, K), generator=g)
    keep, _ = _cuts(ids, E)
    _check(x, ids, w, E, keep, (dtype, vecs))


@pytest.mark.parametrize("vecs", [1, 65])
def test_a_quota_of_the_whole_demand_is_the_unclipped_launch(vecs):
    from mp4x.ops import device_ops as ops
    T, K, E = 150, 2, 5
    x = moe_ref.tokens(T, vecs * 4, torch.float32, 41)
    w = moe_ref.gate_weights(T, K, 42)
    ids = torch.randint(-1, E, (T, K), generator=torch.Generator().manual_seed(43))
    demand = moe_ref.ref_route(ids, E)[0][:E].tolist()
    xd, idd, wd = x.to(DEV), ids.to(DEV), w.to(DEV)
    rc = ops.moe_route_count(idd.reshape(-1), E)
    clip, kept = _clip_table(demand)
    for scale in (None, wd.reshape(-1)):
        plain = torch.empty((kept, vecs * 4), device=DEV)
        clipped = torch.empty((kept, vecs * 4), device=DEV)
        s0 = ops.moe_route_scatter(rc, xd, K, plain, row_scale=scale, placed=kept)
        s1 = ops.moe_route_scatter(rc, xd, K, clipped, row_scale=scale, placed=kept, clip=clip)
        assert torch.equal(s0, s1) and same_bits(plain.cpu(), clipped.cpu())
    _check(x, ids, w, E, demand, ("whole demand", vecs))


def test_the_largest_expert_count_and_empty_quotas():
    E = 2048
    x = moe_ref.tokens(600, 4, torch.float32, 3)
    w = moe_ref.gate_weights(600, 1, 4)
    ids = ((torch.arange(600) * 37) % E).view(600, 1)
    demand = moe_ref.ref_route(ids, E)[0][:E].tolist()
    _check(x, ids, w, E, [d if e % 3 else 0 for e, d in enumerate(demand)], "E = 2048")
    _check(x, ids, w, E, [0] * E, "nothing kept")                # out_rows of no rows but the guard


def test_the_wrapper_refuses_a_bad_table_before_a_launch():
    from mp4x.ops import device_ops as ops
    ids = torch.zeros(8, dtype=torch.int64, device=DEV)
    rc = ops.moe_route_count(ids, 4)
    x = torch.zeros(4, 4, device=DEV)
    out = torch.empty(8, 4, device=DEV)
    good = torch.tensor([3, 0, 0, 0, 0, 3, 3, 3], device=DEV)
    for bad in (good.to(torch.int32), good[:7], good.cpu(), torch.cat([good, good])[::2]):
        with pytest.raises(ValueError):
            ops.moe_route_scatter(rc, x, 2, out, clip=bad)
    with pytest.raises(ValueError):
        ops.moe_route_scatter(rc, x, 2, torch.empty(2, 4, device=DEV), placed=3, clip=good)    # 3 rows are kept
    with pytest.raises(ValueError):
        ops.moe_route_scatter(rc, x, 2, torch.empty(2, 4, device=DEV), clip=good)              # ... read from the table
    slots = ops.moe_route_scatter(rc, x, 2, torch.empty(3, 4, device=DEV), placed=3, clip=good)
    assert slots.cpu().tolist() == [0, 1, 2, -1, -1, -1, -1, -1]
