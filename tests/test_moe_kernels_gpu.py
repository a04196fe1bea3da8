"""The K9 kernels (csrc/kernels/moe.hip) through their device_ops wrappers, one process, against the
contract in tests/moe_ref.py: ``counts`` and ``slots`` exactly, the routed rows, their ``row_scale``
form and the combine bit for bit, both id dtypes, the empty call, and two runs bit-identical."""
import pytest

torch = pytest.importorskip("torch")

import moe_ref  # noqa: E402
from moe_ref import CASES, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _run(x, ids, w, E, scaled):
    """(counts, slots, send rows, combine of the send rows) on the GPU."""
    from mp4x.ops import device_ops as ops
    T, K = ids.shape
    xd, idd, wd = x.to(DEV), ids.to(DEV), w.to(DEV)
    rc = ops.moe_route_count(idd.reshape(-1), E)
    placed = int(rc.counts[:E].sum())
    out = torch.full((placed,) + tuple(x.shape[1:]), 7.0, dtype=x.dtype, device=DEV)
    slots = ops.moe_route_scatter(rc, xd, K, out, row_scale=wd.reshape(-1) if scaled else None)
    comb = ops.moe_combine(out, slots, None if scaled else wd, T, K)
    torch.cuda.synchronize()
    return rc.counts.cpu(), slots.cpu(), out.cpu(), comb.cpu()


def _expect(x, ids, w, E, scaled):
    T, K = ids.shape
    counts, slots, order = moe_ref.ref_route(ids, E)
    send = moe_ref.ref_send(x, order, K, w if scaled else None)
    return counts, slots, send, moe_ref.ref_combine(send, slots, None if scaled else w, T, K)


def _check(x, ids, w, E, what):
    for scaled in (False, True):
        want = _expect(x, ids, w, E, scaled)
        got = _run(x, ids, w, E, scaled)
        again = _run(x, ids, w, E, scaled)
        assert torch.equal(got[0], want[0]), (what, scaled, "counts")
        assert torch.equal(got[1], want[1]), (what, scaled, "slots")
        assert same_bits(got[2], want[2]), (what, scaled, "rows")
        assert same_bits(got[3], want[3]), (what, scaled, "combine")
        assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1]), (what, scaled, "run to run")
        assert same_bits(got[2], again[2]) and same_bits(got[3], again[3]), (what, scaled, "run to run")


@pytest.mark.parametrize("p", [2, 3])
@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case_rank_0(name, p):
    x, ids, w, E = moe_ref.case(name, 0, p)
    _check(x, ids, w, E, (name, p))
    other = torch.int32 if ids.dtype == torch.int64 else torch.int64        # both id dtypes
    _check(x, ids.to(other), w, E, (name, p, other))


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
    _check(x, ids, w, E, (dtype, vecs))


def test_ids_past_the_experts_are_counted_and_placed_nowhere():
    x = moe_ref.tokens(70, 4, torch.float32, 1)
    w = moe_ref.gate_weights(70, 1, 2)
    ids = (torch.arange(70) % 9 - 1).view(70, 1)                             # -1 .. 7 against E = 6
    counts, slots, _, _ = _run(x, ids, w, 6, False)
    assert int(counts[6]) == 8 and int(counts[7]) == int((ids >= 6).sum()) > 0
    assert bool((slots[(ids.reshape(-1) < 0) | (ids.reshape(-1) >= 6)] == -1).all())
    _check(x, ids, w, 6, "past E")


def test_the_largest_expert_count():
    E = 2048
    x = moe_ref.tokens(600, 4, torch.float32, 3)
    w = moe_ref.gate_weights(600, 1, 4)
    ids = ((torch.arange(600) * 37) % E).view(600, 1)
    _check(x, ids, w, E, "E = 2048")


def test_empty_calls():
    from mp4x.ops import device_ops as ops
    ids = torch.empty(0, dtype=torch.int64, device=DEV)
    rc = ops.moe_route_count(ids, 4)
    assert rc.counts.cpu().tolist() == [0] * 6
    x = torch.empty(0, 4, device=DEV)
    out = torch.empty(0, 4, device=DEV)
    slots = ops.moe_route_scatter(rc, x, 3, out)
    assert slots.numel() == 0
    got = ops.moe_combine(out, slots, None, 0, 3)
    assert tuple(got.shape) == (0, 4)
    # tokens whose every assignment is dropped: zeros, from a buffer of no rows
    ids = torch.full((6,), -1, dtype=torch.int32, device=DEV)
    rc = ops.moe_route_count(ids, 4)
    x = torch.ones(3, 4, device=DEV)
    slots = ops.moe_route_scatter(rc, x, 2, out)
    got = ops.moe_combine(out, slots, None, 3, 2)
    assert slots.cpu().tolist() == [-1] * 6 and rc.counts.cpu().tolist() == [0, 0, 0, 0, 6, 0]
    assert same_bits(got, torch.zeros(3, 4))


def test_wrappers_refuse_before_a_launch():
    from mp4x.ops import device_ops as ops
    ids = torch.zeros(8, dtype=torch.int64, device=DEV)
    rc = ops.moe_route_count(ids, 4)
    x = torch.zeros(4, 4, device=DEV)
    with pytest.raises(ValueError):
        ops.moe_route_count(ids.to(torch.int16), 4)
    with pytest.raises(ValueError):
        ops.moe_route_count(ids, 2049)
    with pytest.raises(ValueError):
        ops.moe_route_scatter(rc, x, 2, torch.empty(7, 4, device=DEV))      # 8 rows are placed
    with pytest.raises(ValueError):
        ops.moe_route_scatter(rc, x[:, :3].contiguous(), 2, torch.empty(8, 3, device=DEV))
    with pytest.raises(ValueError):
        ops.moe_route_scatter(rc, x.double(), 2, torch.empty(8, 4, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.moe_route_scatter(rc, x, 3, torch.empty(8, 4, device=DEV))
    slots = torch.tensor([0, 1, 2, 9], device=DEV)
    with pytest.raises(ValueError):
        ops.moe_combine(torch.empty(8, 4, device=DEV), slots, None, 2, 2)   # slot 9 of 8 rows
    with pytest.raises(ValueError):
        ops.moe_combine(torch.empty(8, 4, device=DEV), slots, torch.ones(2, 2, device=DEV, dtype=torch.float64), 2, 2)
