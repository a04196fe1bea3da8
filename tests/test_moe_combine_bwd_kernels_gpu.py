"""K11 (csrc/kernels/moe.hip k_moe_combine_bwd) through ``device_ops.moe_combine_backward``, one
process.  ``g_rows`` has the bits of the K9 route scatter with ``row_scale`` on ids that produce the
same slots (pad rows included in the padded layout); ``g_weights`` is inside the bound of the float64
definition (tests/moe_combine_bwd_ref.py), after the float32 CPU evaluation of the same inputs has
passed it, and +0.0 by bits on clipped assignments.  Every output is pre-filled with NaN and carries
sentinel guard rows behind it that must survive; every launch runs twice and must give the same bits."""
import pytest

torch = pytest.importorskip("torch")

import moe_combine_bwd_ref as ref  # noqa: E402
from moe_ref import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD, SENTINEL, SPARE = 3, 1024.0, 2
TS, KS, VS = (1, 63, 64, 65, 300), (1, 2, 8, 16), (1, 2, 3, 5, 64, 65, 130)
DTYPES = ("float32", "bfloat16", "float16")
NB = 5                       # experts of the ids; the padded layout has NB + 3 blocks, three of them all pad
WORST = {}


def _guarded(rows, tail, dtype):
    buf = torch.full((rows + GUARD,) + tail, float("nan"), dtype=dtype, device=DEV)
    buf[rows:] = SENTINEL
    return buf


def _guards_ok(buf, rows):
    return buf.shape[0] == rows + GUARD and bool((buf[rows:] == SENTINEL).all())


def _reference_scatter(g, ids, w, K, share):
    """(slots on the device, the rows the K9 scatter writes with row_scale = w, NaN where it writes
    nothing).  Ragged: SPARE rows more than are placed, which no slot names."""
    from mp4x.ops import device_ops as ops
    if share is None:
        rc = ops.moe_route_count(ids, NB)
        placed = int(rc.counts[:NB].sum())
        rows = torch.full((placed + SPARE,) + tuple(g.shape[1:]), float("nan"), dtype=g.dtype, device=DEV)
        return ops.moe_route_scatter(rc, g, K, rows, row_scale=w, placed=placed), rows, None
    rc = ops.moe_route_count(ids, NB + 3)
    rows = torch.full(((NB + 3) * share,) + tuple(g.shape[1:]), float("nan"), dtype=g.dtype, device=DEV)
    return ops.moe_route_scatter_pad(rc, g, K, rows, share, row_scale=w), rows, (rc, share)


def _launch(g, rows, slots, w, T, K, pad):
    from mp4x.ops import device_ops as ops
    g_rows, g_w = _guarded(rows.shape[0], tuple(rows.shape[1:]), rows.dtype), _guarded(T, (K,), torch.float32)
    out = ops.moe_combine_backward(g, rows, slots, w, T, K, out=(g_rows[:rows.shape[0]], g_w[:T]), pad=pad)
    assert out[0].data_ptr() == g_rows.data_ptr() and out[1].data_ptr() == g_w.data_ptr()
    torch.cuda.synchronize()
    return g_rows[:rows.shape[0]].cpu(), g_w[:T].cpu(), _guards_ok(g_rows, rows.shape[0]) and _guards_ok(g_w, T)


def _check(g, rows_of, ids, w, K, share, what, want_slots=None):
    """``rows_of(n)``: the n slot rows (the combine's input) of the case."""
    T = g.shape[0]
    gd, wd = g.to(DEV), w.to(DEV)
    slots, want_rows, pad = _reference_scatter(gd, ids.to(DEV), wd, K, share)
    rows = rows_of(want_rows.shape[0])
    sl = slots.cpu()
    if want_slots is not None:
        assert torch.equal(sl, want_slots), (what, "slots")
    live = sl[sl >= 0]
    assert live.numel() == live.unique().numel() and (live.numel() == 0 or int(live.max()) < rows.shape[0]), what
    want64, bound = ref.definition(g, rows, sl, K)
    ok, ratio = ref.inside(ref.torch_f32(g, rows, sl, K), want64, bound)
    assert ok, (what, "the float32 CPU evaluation", ratio)
    got = _launch(gd, rows.to(DEV), slots, wd, T, K, pad)
    again = _launch(gd, rows.to(DEV), slots, wd, T, K, pad)
    assert got[2] and again[2], (what, "guard rows")
    assert same_bits(got[0], again[0]) and same_bits(got[1], again[1]), (what, "run to run")
    assert same_bits(got[0], want_rows.cpu()), (what, "g_rows against the route scatter with row_scale")
    if share is None:
        assert bool(torch.isnan(got[0][want_rows.shape[0] - SPARE:]).all()), (what, "rows no slot names")
    else:
        named = torch.zeros(rows.shape[0], dtype=torch.bool)
        named[live] = True
        assert bool((got[0][~named].view(torch.uint8) == 0).all()), (what, "pad rows are zero bits")
    ok, ratio = ref.inside(got[1], want64, bound)
    WORST[what[-1]] = max(WORST.get(what[-1], 0.0), ratio)
    print(what, "g_weights worst / bound = %.3f" % ratio)
    assert ok, (what, "g_weights", ratio)
    assert ref.zero_bits_where_clipped(got[1], sl), (what, "clipped assignments are +0.0")
    return sl


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", VS)
def test_shapes_layouts_and_bounds(V, dtype):
    dt = getattr(torch, dtype)
    width = V * 16 // torch.empty((), dtype=dt).element_size()
    WORST.pop(dtype, None)
    for n, (T, K) in enumerate((T, K) for T in TS for K in KS):
        kind = ("ragged", "clipped", "padded")[(n + V) % 3]
        seed = 10000 * V + 10 * n
        ids = ref.clipped_ids(T, K, NB, seed) if kind == "clipped" else ref.ragged_ids(T, K, NB, seed)
        share = T * K // (NB + 1) + 1 if kind == "padded" else None       # below T * K / NB: some expert is cut
        want_slots = ref.padded_slots(ids, NB + 3, share) if share else ref.ragged_slots(ids, NB)[0]
        if share:
            assert (NB + 3) * share > T * K                  # slots past T * K
        g, w = ref.values(T, width, dt, seed + 1), ref.weights(T, K, seed + 2)
        _check(g, lambda rows: ref.values(rows, width, dt, seed + 3), ids, w, K, share, (T, K, V, kind, dtype), want_slots)
    print("largest g_weights worst / bound for", dtype, "V =", V, ": %.3f" % WORST[dtype])


@pytest.mark.parametrize("dtype", DTYPES)
def test_products_that_cancel_are_bounded_by_the_sum_of_magnitudes(dtype):
    dt = getattr(torch, dtype)
    for T, width in ((65, 64), (300, 1040)):
        g, rows, slots = ref.cancelling(T, width, dt, 77 + T)
        ids = torch.tensor([[0, 1]] * T)                   # expert 0 then expert 1 of every token: slots t and T + t
        spare = ref.values(SPARE, width, dt, 5)
        sl = _check(g, lambda n: torch.cat([rows, spare])[:n], ids, ref.weights(T, 2, 78), 2, None,
                    (T, 2, width, "cancelling", dtype), slots)
        want64, bound = ref.definition(g, rows, sl, 2)
        assert bool((want64[:, 0] == 0).all()) and bool((bound[:, 0] > 0).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_clipped_assignments_read_nothing(dtype):
    from mp4x.ops import device_ops as ops
    dt = getattr(torch, dtype)
    T, K, width = 65, 8, 72
    g, w = ref.values(T, width, dt, 1).to(DEV), ref.weights(T, K, 2).to(DEV)
    rows = torch.full((7, width), float("nan"), dtype=dt, device=DEV)
    slots = torch.full((T * K,), -1, dtype=torch.int64, device=DEV)
    g_rows, g_w, guards = _launch(g, rows, slots, w, T, K, None)
    assert guards and bool(torch.isnan(g_rows).all())
    assert bool((g_w.view(torch.int32) == 0).all())
    # one live slot among them: its row is the only one written
    slots[3 * K + 5] = 4
    rows[4] = ref.values(1, width, dt, 3).to(DEV)[0]
    g_rows, g_w, guards = _launch(g, rows, slots, w, T, K, None)
    assert guards and bool(torch.isnan(g_rows[[0, 1, 2, 3, 5, 6]]).all())
    assert same_bits(g_rows[4], (w[3, 5].cpu() * g[3].cpu().to(torch.float32)).to(dt))
    assert int((g_w.view(torch.int32) != 0).sum()) == 1 and float(g_w[3, 5]) != 0.0
    # no rows at all (nothing was placed) and no token
    none = ops.moe_combine_backward(g, rows[:0], torch.full_like(slots, -1), w, T, K)
    assert none[0].shape == (0, width) and bool((none[1].cpu().view(torch.int32) == 0).all())
    empty = ops.moe_combine_backward(g[:0], rows, slots[:0], w[:0], 0, K)
    assert empty[0].shape == rows.shape and empty[1].shape == (0, K)


def test_refusals_leave_every_output_as_it_was():
    from mp4x.operators import DType
    from mp4x.ops import device_ops as ops, native
    lib = native.hip()
    T, K, width, R = 4, 2, 8, 8
    g = torch.zeros(T, width, device=DEV)
    rows = torch.full((R + GUARD, width), float("nan"), device=DEV)
    g_rows, g_w = _guarded(R, (width,), torch.float32), _guarded(T, (17,), torch.float32)
    slots = torch.arange(T * 17, dtype=torch.int64, device=DEV) % R
    w = torch.ones(T * 17, device=DEV)
    before = [t.clone() for t in (rows, g_rows, g_w)]

    def call(dtype=int(DType.F32), K=K, width=width, rows=rows.data_ptr(), g_rows=g_rows.data_ptr(), g_w=g_w.data_ptr()):
        return lib.mp4x_moe_combine_backward(dtype, g.data_ptr(), rows, R, slots.data_ptr(), w.data_ptr(), T, K, width,
                                             g_rows, g_w, None)

    bad = native.E_BADARG
    assert call(K=17) == bad                                                  # past the kernel's K
    assert call(dtype=int(DType.BF16), width=4) == bad                        # a row of 8 bytes
    assert call(g_w=g_w.data_ptr() + 2) == bad                                # a misaligned g_weights
    assert call(g_rows=rows.data_ptr()) == bad                                # g_rows aliasing rows ...
    assert call(g_rows=rows.data_ptr() + (R - 1) * width * 4) == bad          # ... or only its last row
    assert call(g_rows=g.data_ptr()) == bad and call(dtype=int(DType.F64)) == native.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(same_bits(a.cpu(), b.cpu()) for a, b in zip((rows, g_rows, g_w), before))
    sl, wt = slots[:T * K].contiguous(), w[:T * K].contiguous()
    for bad_call in (lambda: ops.moe_combine_backward(g, rows[:R], slots, w, T, 17),
                     lambda: ops.moe_combine_backward(g, rows[:R], sl, wt, T, 0),
                     lambda: ops.moe_combine_backward(g.double(), rows[:R].double(), sl, wt, T, K),
                     lambda: ops.moe_combine_backward(g[:, :2].contiguous(), rows[:R, :2].contiguous(), sl, wt, T, K),
                     lambda: ops.moe_combine_backward(g, rows[:R].half(), sl, wt, T, K),
                     lambda: ops.moe_combine_backward(g, rows[:R], sl + R, wt, T, K),
                     lambda: ops.moe_combine_backward(g, rows[:R], sl, wt.double(), T, K),
                     lambda: ops.moe_combine_backward(g, rows[:R], sl.int(), wt, T, K),
                     lambda: ops.moe_combine_backward(g.cpu(), rows[:R], sl, wt, T, K),
                     lambda: ops.moe_combine_backward(g, rows[:R], sl, wt, T, K, out=(g_rows[:R - 1], g_w[:T, :K]))):
        with pytest.raises(ValueError, match="moe_combine_backward|device op"):
            bad_call()
