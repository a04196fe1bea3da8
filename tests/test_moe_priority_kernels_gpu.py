"""The K15 kernels (csrc/kernels/moe_priority.hip) behind ``device_ops.moe_priority_mask``, one process,
against the plain-Python definition of tests/moe_priority_ref.py.  Everything is integers: every
comparison is exact.  Shapes are the smallest at which the kernels can go wrong: a tile tail (n = 111),
three 256-tiles (n = 600, ties that straddle tile borders), one expert / a few / 64 / 2048 (most empty),
a limit vector holding 0, cnt - 1, cnt, cnt + 1 and a huge value, a scalar limit of 1, everything to
one expert, stray ids, and priorities that make single passes of the radix select decide: constant
(the index bytes alone), last-mantissa-bit neighbours, +-0 / +-inf / both NaNs / denormals.  n = 65 600
with a constant priority is the only case that reaches the third index byte.  ``out`` carries sentinel
guard elements that must survive; every call runs twice and must give the same bits."""
import pytest

torch = pytest.importorskip("torch")

import moe_priority_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD, SENTINEL = 5, -77


def _run(ids, prio, nb, limit):
    from mp4x.ops import device_ops as ops
    n = ids.numel()
    idd, pd = ids.to(DEV), prio.to(DEV)
    lim = limit.to(DEV) if isinstance(limit, torch.Tensor) else limit
    rc = ops.moe_route_count(idd, nb)
    buf = torch.full((n + GUARD,), SENTINEL, dtype=ids.dtype, device=DEV)
    out, masked = ops.moe_priority_mask(rc, pd, lim, out=buf[:n])
    fresh, masked2 = ops.moe_priority_mask(rc, pd, lim)
    torch.cuda.synchronize()
    assert out.data_ptr() == buf.data_ptr() and masked.dtype == torch.int64 and tuple(masked.shape) == (1,)
    assert bool((buf[n:] == SENTINEL).all()), "guard elements"
    assert torch.equal(fresh, out) and torch.equal(masked, masked2), "the same call twice"
    assert torch.equal(idd.cpu(), ids), "the ids are untouched"
    return out.cpu(), int(masked)


def _check(ids, prio, nb, limit, what):
    want, want_masked = ref.mask_tensors(ids, prio, nb, limit)
    got, masked = _run(ids, prio, nb, limit)
    assert got.dtype == ids.dtype
    assert torch.equal(got, want), (what, (got != want).nonzero().reshape(-1)[:8].tolist())
    assert masked == want_masked == int(((got == -1) & (ids != -1)).sum()), what
    return got


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("n,nb", ref.SHAPES)
def test_the_kernels_equal_the_definition(n, nb, kind):
    ids = ref.ids_for(n, nb, 17 * n + nb)
    prio = ref.priorities(kind, n, n + nb)
    for idt in (torch.int64, torch.int32):
        _check(ids.to(idt), prio, nb, ref.limit_vector(ids, nb, nb), (n, nb, kind, idt, "vector"))
        _check(ids.to(idt), prio, nb, 1, (n, nb, kind, idt, "scalar 1"))


@pytest.mark.parametrize("kind", ref.KINDS)
def test_all_assignments_to_one_expert(kind):
    ids = torch.full((600,), 2, dtype=torch.int64)
    got = _check(ids, ref.priorities(kind, 600, 5), 3, 5, kind)
    assert int((got == 2).sum()) == 5


def test_a_constant_priority_is_the_position_policy():
    n, nb = 600, 3
    ids = ref.ids_for(n, nb, 31)
    lim = ref.limit_vector(ids, nb, 1)
    got, _ = _run(ids, ref.priorities("constant", n, 0), nb, lim)
    assert got.tolist() == ref.position_mask(ids.tolist(), nb, lim.tolist())


@pytest.mark.parametrize("limit", [40000, 1])
def test_the_third_index_byte(limit):
    T, K = 8200, 8
    n = T * K                               # 65 600 > 2^16 assignments, two experts, one priority
    ids = (torch.arange(n) % 3 == 0).to(torch.int32)
    got = _check(ids, ref.priorities("constant", n, 0), 2, limit, limit)
    assert got.tolist() == ref.position_mask(ids.tolist(), 2, limit)


def test_no_assignment_at_all():
    from mp4x.ops import device_ops as ops
    ids = torch.empty(0, dtype=torch.int64, device=DEV)
    rc = ops.moe_route_count(ids, 4)
    out, masked = ops.moe_priority_mask(rc, torch.empty(0, device=DEV), 3)
    assert out.numel() == 0 and masked.tolist() == [0]


def test_the_wrapper_refuses_before_any_launch():
    from mp4x.ops import device_ops as ops
    ids = ref.ids_for(64, 4, 1).to(DEV)
    rc = ops.moe_route_count(ids, 4)
    p = torch.rand(64, device=DEV)
    for bad in (dict(priority=p.double()), dict(priority=p[:63]), dict(priority=p.cpu()), dict(limit=-1), dict(limit=True),
                dict(limit=2.0), dict(limit=torch.ones(4, dtype=torch.int32, device=DEV)),
                dict(limit=torch.ones(5, dtype=torch.int64, device=DEV)), dict(limit=torch.ones(4, dtype=torch.int64)),
                dict(out=ids), dict(out=torch.empty(64, dtype=torch.int32, device=DEV)),
                dict(out=torch.empty(63, dtype=torch.int64, device=DEV))):
        kw = dict(priority=p, limit=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.moe_priority_mask(rc, kw["priority"], kw["limit"], out=kw.get("out"))
