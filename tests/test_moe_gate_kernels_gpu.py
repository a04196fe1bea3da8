"""K10 (csrc/kernels/moe_gate.hip) through ``device_ops``, one process, against the float64 definition
of tests/moe_gate_ref.py: ids and counts exactly, weights / lse / prob_sum / g_logits inside the derived
bounds (DESIGN "K10"; the 16-bit rounding term as corrected in tests/test_moe_gate_cpu.py), each
after the float32 CPU evaluation of the same inputs has passed the same bound.  Every output buffer
is pre-filled with NaN (-1 for ids) and carries sentinel guard rows behind it that must survive;
every launch runs twice and must give the same bits."""
import pytest

torch = pytest.importorskip("torch")

import moe_gate_ref as ref  # noqa: E402
from moe_ref import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD, SENTINEL, ID_SENTINEL = 3, 1024.0, -7
TS, KS = (1, 63, 64, 65, 300), (1, 2, 8, 16)
DTYPES = ("float32", "bfloat16", "float16")


def _guarded(rows, tail, dtype):
    fill, guard = (-1, ID_SENTINEL) if dtype in (torch.int32, torch.int64) else (float("nan"), SENTINEL)
    buf = torch.full((rows + GUARD,) + tail, fill, dtype=dtype, device=DEV)
    buf[rows:] = guard
    return buf


def _guards_ok(bufs, rows):
    return all(bool((b[n:] == (ID_SENTINEL if b.dtype in (torch.int32, torch.int64) else SENTINEL)).all())
               and b.shape[0] == n + GUARD for b, n in zip(bufs, rows))


def _run(logits, K, renormalize, ids_dtype, grads=None):
    """One forward with the statistics and one backward: (weights, ids, lse, prob_sum, counts,
    g_logits) on the host and whether every guard row survived."""
    from mp4x.ops import device_ops as ops
    T, E = logits.shape
    ld = logits.to(DEV)
    bufs = [_guarded(T, (K,), torch.float32), _guarded(T, (K,), ids_dtype), _guarded(T, (), torch.float32),
            _guarded(E, (), torch.float32), _guarded(E, (), torch.int64), _guarded(T, (E,), logits.dtype)]
    rows = [T, T, T, E, E, T]
    out = tuple(b[:n] for b, n in zip(bufs[:5], rows))
    got = ops.moe_gate_topk(ld, K, renormalize, ids_dtype, stats=True, out=out)
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
    gd = [None if g is None else g.to(DEV) for g in (grads or (None, None, None))]
    ops.moe_gate_backward(ld, got[2], got[1], renormalize, *gd, out=bufs[5][:T])
    torch.cuda.synchronize()
    return [b[:n].cpu() for b, n in zip(bufs, rows)], _guards_ok(bufs, rows)


def _check(logits, want, K, renormalize, ids_dtype, grads, what, values=True):
    cpu = None
    if values:                                        # the float32 CPU evaluation is inside the bounds first
        from mp4x.models.moe import gate_backward_torch, gate_forward_torch
        cw, cids, clse, cps, _ = gate_forward_torch(logits, K, renormalize, torch.int64, True)
        cpu = (cw, cids, clse, cps, None, gate_backward_torch(logits, clse, cids, renormalize, *grads))
    got, guards = _run(logits, K, renormalize, ids_dtype, grads)
    again, guards2 = _run(logits, K, renormalize, ids_dtype, grads)
    assert guards and guards2, (what, "guard rows")
    assert got[1].dtype == ids_dtype and torch.equal(got[1].to(torch.int64), want.ids), (what, "ids")
    assert torch.equal(got[4], want.counts), (what, "counts")
    for a, b in zip(got, again):
        assert same_bits(a, b) if a.is_floating_point() else torch.equal(a, b), (what, "run to run")
    if not values:
        return
    g64, gbound = want.backward(*grads)
    for name, i, w64, bound in (("weights", 0, want.w, want.weights_bound()), ("lse", 2, want.lse, want.lse_bound()),
                                ("prob_sum", 3, want.prob_sum, want.prob_sum_bound()), ("g_logits", 5, g64, gbound)):
        ok, ratio = ref.inside(cpu[i], w64, bound)
        assert ok, (what, name, "the float32 CPU evaluation", ratio)
        ok, ratio = ref.inside(got[i], w64, bound)
        print(what, name, "worst / bound = %.3f" % ratio)
        assert ok, (what, name, ratio)


def _shapes(E):
    ks = sorted({min(k, E) for k in KS})
    if E <= 128:
        return [(T, K) for T in TS for K in ks]
    return [(T, ks[i % len(ks)]) for i, T in enumerate(TS)] + [(300, K) for K in ks]     # long rows: every T and every K once


@pytest.mark.parametrize("E", [1, 2, 5, 8, 60, 64, 65, 128, 257, 2048])
def test_shapes_dtypes_and_bounds(E):
    for n, (T, K) in enumerate(_shapes(E)):
        for dtype in (DTYPES if E <= 8 else (DTYPES[n % 3],)):
            renormalize, R = bool((n + T) % 2), (4, 32)[n % 2]
            which = ref.GRAD_SETS[1 + n % 7]                       # every set of present gradients but the empty one
            logits, want = ref.cached_reference("uniform", T, E, K, renormalize, R, 1000 + E + n, dtype)
            grads = ref.pick(ref.gradients(T, E, K, 2000 + E + n), which)
            _check(logits, want, K, renormalize, (torch.int64, torch.int32)[n % 2], grads, (T, E, K, dtype, renormalize, R))


@pytest.mark.parametrize("dtype", DTYPES)
def test_both_renormalisations_with_every_gradient(dtype):
    for E, K in ((8, 2), (64, 8), (257, 16)):
        for renormalize in (False, True):
            logits, want = ref.cached_reference("uniform", 65, E, K, renormalize, 4, 3000 + E, dtype)
            _check(logits, want, K, renormalize, torch.int64, ref.gradients(65, E, K, 3100 + E), (E, K, dtype, renormalize))
    logits, want = ref.cached_reference("uniform", 65, 64, 8, False, 4, 3064, dtype)
    _check(logits, want, 8, False, torch.int32, (None, None, None), (dtype, "no gradient at all"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_ids_on_ties_and_masks_equal_the_stable_sort(dtype):
    for E in (1, 2, 5, 8, 60, 64, 65, 128, 257, 2048):
        for n, K in enumerate(sorted({min(k, E) for k in KS})):
            renormalize = bool(n % 2)
            logits, want = ref.cached_reference("ties", 65, E, K, renormalize, 0, 500 + E, dtype)
            grads = ref.gradients(65, E, K, 4000 + E)
            _check(logits, want, K, renormalize, (torch.int64, torch.int32)[n % 2], grads, ("ties", E, K, dtype))


def test_any_bits_give_ids_in_range_and_distinct():
    nan, inf = float("nan"), float("inf")
    for E, K in ((5, 5), (64, 8), (257, 16), (2048, 16)):
        lg = ref.uniform_logits(9, E, 4, 77)
        lg[0] = nan
        lg[1] = inf
        lg[2] = -inf
        lg[3, ::2] = nan
        lg[4, 1::3] = inf
        lg[5] = torch.tensor([0x7fffffff, -1, 0x7f800001, -8388607], dtype=torch.int32).view(torch.float32).repeat(E)[:E]
        lg[6, :E // 2] = -nan
        for dtype in DTYPES:
            for ids_dtype in (torch.int64, torch.int32):
                got, guards = _run(lg.to(getattr(torch, dtype)), K, True, ids_dtype, ref.gradients(9, E, K, 78))
                ids = got[1].to(torch.int64)
                assert guards, (E, dtype)
                assert bool(((ids >= 0) & (ids < E)).all()), (E, dtype)
                assert all(len(set(row)) == K for row in ids.tolist()), (E, dtype)
                assert torch.equal(got[4], torch.bincount(ids.reshape(-1), minlength=E)), (E, dtype)
                assert torch.equal(ids[7:], ref.order_ids(lg.to(getattr(torch, dtype))[7:], K)), (E, dtype)


def test_no_token():
    from mp4x.ops import device_ops as ops
    lg = torch.empty(0, 7, device=DEV)
    w, ids, lse, ps, cnt = ops.moe_gate_topk(lg, 3, stats=True)
    assert w.shape == (0, 3) and ids.shape == (0, 3) and lse.shape == (0,)
    assert ps.cpu().tolist() == [0.0] * 7 and cnt.cpu().tolist() == [0] * 7
    assert ops.moe_gate_topk(lg, 3)[3:] == (None, None)
    assert ops.moe_gate_backward(lg, lse, ids).shape == (0, 7)


def test_refusals_return_their_codes_without_a_launch():
    from mp4x.operators import DType
    from mp4x.ops import device_ops as ops, native
    lib = native.hip()
    T, E, K = 4, 8, 2
    lg = torch.zeros(T + 1, E, device=DEV)
    bufs = [_guarded(T, (K,), torch.float32), _guarded(T, (K,), torch.int64), _guarded(T, (), torch.float32),
            _guarded(E, (), torch.float32), _guarded(E, (), torch.int64), _guarded(T, (E,), torch.float32)]
    scratch = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    before = [b.clone() for b in bufs]

    def fwd(dtype=int(DType.F32), logits=lg.data_ptr(), T=T, E=E, K=K, w=bufs[0].data_ptr(), ids=bufs[1].data_ptr(),
            lse=bufs[2].data_ptr(), ps=bufs[3].data_ptr(), cnt=bufs[4].data_ptr(), sc=scratch.data_ptr(), sb=1 << 16):
        return lib.mp4x_moe_gate_topk(dtype, logits, T, E, K, 0, w, ids, 1, lse, ps, cnt, sc, sb, None)

    def bwd(dtype=int(DType.F32), logits=lg.data_ptr(), T=T, E=E, K=K, out=bufs[5].data_ptr(), ids=bufs[1].data_ptr()):
        return lib.mp4x_moe_gate_backward(dtype, logits, bufs[2].data_ptr(), ids, 1, T, E, K, 0, None, None, None, out, None)

    bad, uns = native.E_BADARG, native.E_UNSUPPORTED
    for f in (fwd, bwd):
        assert [f(E=0), f(E=2049), f(K=0), f(K=17), f(E=8, K=9), f(T=-1)] == [bad] * 6
        assert [f(dtype=int(d)) for d in (DType.F64, DType.I32, DType.U8)] == [uns] * 3 and f(dtype=99) == uns
        assert f(logits=lg.data_ptr() + 4) == bad and f(logits=None) == bad and f(ids=bufs[1].data_ptr() + 4) == bad
    assert fwd(w=bufs[0].data_ptr() + 2) == bad and fwd(lse=None) == bad
    assert fwd(cnt=None) == bad and fwd(ps=None) == bad                      # the statistics: both or neither
    assert fwd(sc=scratch.data_ptr() + 16) == bad and fwd(sb=8) == bad and fwd(sc=None) == bad
    assert bwd(out=bufs[5].data_ptr() + 4) == bad and bwd(out=None) == bad
    assert lib.mp4x_moe_gate_scratch_bytes(int(DType.F64), 4, 8) == 0 and lib.mp4x_moe_gate_scratch_bytes(1, 4, 0) == 0
    torch.cuda.synchronize()
    assert all(same_bits(a, b) if a.is_floating_point() else torch.equal(a, b) for a, b in zip(bufs, before))
    # the wrappers refuse with the function's name
    for call in (lambda: ops.moe_gate_topk(lg, 0), lambda: ops.moe_gate_topk(lg, 9), lambda: ops.moe_gate_topk(lg, 17),
                 lambda: ops.moe_gate_topk(lg.double(), 2), lambda: ops.moe_gate_topk(lg.cpu(), 2),
                 lambda: ops.moe_gate_topk(lg[:, :4], 2), lambda: ops.moe_gate_topk(lg, 2, ids_dtype=torch.int16),
                 lambda: ops.moe_gate_topk(torch.zeros(2, 2049, device=DEV), 2),
                 lambda: ops.moe_gate_topk(lg, 2, out=(bufs[0],) * 5)):
        with pytest.raises(ValueError, match="moe_gate_topk|device op"):
            call()
    ids = torch.zeros(T + 1, K, dtype=torch.int64, device=DEV)
    lse = torch.zeros(T + 1, device=DEV)
    for call in (lambda: ops.moe_gate_backward(lg, lse[:2], ids), lambda: ops.moe_gate_backward(lg, lse, ids[:2]),
                 lambda: ops.moe_gate_backward(lg, lse, ids.float()), lambda: ops.moe_gate_backward(lg, lse.double(), ids),
                 lambda: ops.moe_gate_backward(lg, lse, ids, g_prob_sum=torch.zeros(E + 1, device=DEV)),
                 lambda: ops.moe_gate_backward(lg, lse, ids, out=torch.zeros(T + 1, E, device=DEV, dtype=torch.float16))):
        with pytest.raises(ValueError, match="moe_gate_backward"):
            call()
