"""The definition of the grouped expert GEMM (``mp4x.parallel.moe.grouped_mm_torch`` /
``grouped_mm_wgrad_torch``) against the float64 definition and bound of tests/moe_gemm_ref.py in both
segment layouts, pad rows that come out +0 and are never read, ``TokenPlan.segment_table`` and the
refusals.  No GPU."""
import pytest

torch = pytest.importorskip("torch")

import moe_gemm_ref as ref  # noqa: E402
from moe_gemm_ref import same_bits  # noqa: E402

LAYOUTS = (lambda: ref.ragged([0, 17, 5, 1, 40], 3), lambda: ref.ragged([9, 0], 0), lambda: ref.ragged([0, 0], 4),
           lambda: ref.padded([[0, 1, 7], [8, 9, 300], [0, 0, 0]], 8), lambda: ref.padded([[3, 11]], 11))


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("layout", range(len(LAYOUTS)))
def test_the_torch_form_is_the_definition(layout, dtype):
    from mp4x.parallel.moe import grouped_mm_torch, grouped_mm_wgrad_torch
    dt = getattr(torch, dtype)
    table, R, segs = LAYOUTS[layout]()
    G, Kd, N = len(segs), 24, 40
    keep = ref.owned(segs, R)
    nan = float("nan")
    x, gy, mk = (ref.poison(ref.values((R, w), dt, 5 + w), keep, nan) for w in (Kd, N, N + 0))
    W, Wt, bias = ref.values((G, Kd, N), dt, 1), ref.values((G, N, Kd), dt, 2), ref.values((G, N), dt, 3)
    for tw, b, act, m in ((False, bias, "relu", None), (False, None, None, None), (True, None, None, mk),
                          (True, bias, "relu", mk)):
        w = Wt if tw else W
        got = grouped_mm_torch(ref.shaped(x, table), w, table, b, act, tw, None if m is None else ref.shaped(m, table))
        assert got.dtype == dt and got.shape == ref.shaped(x, table).shape[:-1] + (N,)
        want, bound = ref.forward(x, w, segs, b, act, tw, m)
        ok, ratio = ref.inside(got, want, bound, dt)
        assert ok, (tw, act, ratio)
        flat = got.reshape(-1, N)
        assert bool((flat[~keep].contiguous().view(torch.uint8) == 0).all())          # pad rows are +0 by bits
        assert bool(torch.isfinite(flat.to(torch.float32)).all())
    gw, gb = grouped_mm_wgrad_torch(ref.shaped(x, table), ref.shaped(gy, table), table)
    gw64, bw, gb64, bb = ref.wgrad(x, gy, segs)
    assert gw.dtype == dt and gw.shape == (G, Kd, N) and gb.shape == (G, N)
    assert ref.inside(gw, gw64, bw, dt)[0] and ref.inside(gb, gb64, bb, dt)[0]
    assert grouped_mm_wgrad_torch(ref.shaped(x, table), ref.shaped(gy, table), table, want_bias=False)[1] is None
    for g, group in enumerate(segs):
        if sum(n for _, n in group) == 0:
            assert bool((gw[g].contiguous().view(torch.uint8) == 0).all()) and bool((gb[g] == 0).all())


def test_the_bound_is_a_bound_not_a_tolerance():
    table, R, segs = ref.ragged([6, 3])
    x, W = ref.values((R, 16), torch.float32, 1), ref.values((2, 16, 8), torch.float32, 2)
    want, bound = ref.forward(x, W, segs)
    assert bool((bound > 0).all()) and ref.inside(want.to(torch.float32), want, bound, torch.float32)[0]
    assert not ref.inside((want + 3 * bound + 1e-6).to(torch.float32), want, bound, torch.float32)[0]
    # integer data: float32 sums are exact, the definition rounds once
    xi, Wi = ref.integers((R, 16), 0, 7, 2, torch.bfloat16), ref.integers((2, 16, 8), 1, 3, 5, torch.bfloat16)
    from mp4x.parallel.moe import grouped_mm_torch
    assert same_bits(grouped_mm_torch(xi, Wi, table), ref.forward(xi, Wi, segs)[0].to(torch.bfloat16))
    assert not torch.equal(Wi[0, :8, :8], Wi[0, :8, :8].t())


def test_segment_table_of_a_plan():
    from mp4x.parallel.moe import TokenPlan
    slots = torch.zeros(4, dtype=torch.int64)
    kind, offsets = TokenPlan(expert_counts=(3, 0, 2), slots=slots).segment_table()
    assert kind == "ragged" and offsets.dtype == torch.int64 and offsets.tolist() == [0, 3, 3, 5]
    valid = torch.tensor([[1, 2], [0, 3]])
    table = TokenPlan(expert_counts=(6, 6), slots=slots, source_capacity=3, valid=valid).segment_table()
    assert table[0] == "padded" and table[1] is valid and table[2] == 3
    assert "segment_table" not in TokenPlan.__slots__


def test_unknown_values_raise():
    from mp4x.parallel.moe import grouped_mm_torch, grouped_mm_wgrad_torch
    table, R, _ = ref.ragged([2, 1])
    x, W = torch.zeros(R, 4), torch.zeros(2, 4, 4)
    with pytest.raises(ValueError, match="act"):
        grouped_mm_torch(x, W, table, act="silu")
    for bad in (("ragged",), ("dense", table[1]), ("ragged", table[1][:2]), ("padded", torch.zeros(2, 2), 0), None):
        with pytest.raises(ValueError, match="table"):
            grouped_mm_torch(x, W, bad)
    with pytest.raises(ValueError, match="table"):
        grouped_mm_torch(x, W, ("padded", torch.zeros(2, 2, dtype=torch.int64), 3))        # rows are not [2, 6, 4]
    with pytest.raises(ValueError, match="table"):
        grouped_mm_wgrad_torch(x, x, ("padded", torch.zeros(2, 2, dtype=torch.int64), 3))
