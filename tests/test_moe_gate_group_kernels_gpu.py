"""K13 (csrc/kernels/moe_gate_group.hip) through ``device_ops``, one process, against the float64
definition of tests/moe_gate_group_ref.py: the selection by the tolerance-aware check everywhere and
exactly on the separated fixtures, counts exactly, weights / lse / prob_sum / g_logits inside the
derived bounds (DESIGN "K13"), each after the float32 CPU evaluation of the same inputs has passed
the same bound; without a bias and with one group the ids are K10's.  Every output buffer is
pre-filled with NaN (-1 for ids) and carries sentinel guard rows behind it that must survive; every
launch runs twice and must give the same bits."""
import pytest

torch = pytest.importorskip("torch")

import moe_gate_group_ref as ref  # noqa: E402
import moe_gate_ref  # noqa: E402
from moe_ref import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD, SENTINEL, ID_SENTINEL = 3, 1024.0, -7
TS = (1, 63, 64, 65, 300)
DTYPES = ("float32", "bfloat16", "float16")
# (E, Gr, Kg, K): every lane-group width (G = 1 ... 64), whole-vector and scalar loads
SHAPES = [(8, 4, 2, 2), (6, 3, 2, 4), (60, 5, 3, 6), (64, 8, 4, 8), (64, 1, 1, 8), (256, 8, 4, 8), (260, 4, 1, 16),
          (2048, 32, 8, 16)]


def _guarded(rows, tail, dtype):
    fill, guard = (-1, ID_SENTINEL) if dtype in (torch.int32, torch.int64) else (float("nan"), SENTINEL)
    buf = torch.full((rows + GUARD,) + tail, fill, dtype=dtype, device=DEV)
    buf[rows:] = guard
    return buf


def _guards_ok(bufs, rows):
    return all(bool((b[n:] == (ID_SENTINEL if b.dtype in (torch.int32, torch.int64) else SENTINEL)).all())
               and b.shape[0] == n + GUARD for b, n in zip(bufs, rows))


def _run(logits, bias, K, score, Gr, Kg, renormalize, scale, ids_dtype, grads=None):
    """One forward with the statistics and one backward: [weights, ids, lse, prob_sum, counts,
    group_ids, g_logits] on the host (lse None for the sigmoid) and whether every guard row survived."""
    from mp4x.ops import device_ops as ops
    T, E = logits.shape
    ld = logits.to(DEV)
    bufs = [_guarded(T, (K,), torch.float32), _guarded(T, (K,), ids_dtype), _guarded(T, (), torch.float32),
            _guarded(E, (), torch.float32), _guarded(E, (), torch.int64), _guarded(T, (Kg,), torch.int32),
            _guarded(T, (E,), logits.dtype)]
    rows = [T, T, T, E, E, T, T]
    out = [b[:n] for b, n in zip(bufs[:6], rows)]
    if score == "sigmoid":
        out[2] = None
    got = ops.moe_gate_group_topk(ld, K, score, None if bias is None else bias.to(DEV), Gr, Kg, renormalize, scale,
                                  ids_dtype, stats=True, out=tuple(out))
    assert all((g is None and o is None) or g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
    gd = [None if g is None else g.to(DEV) for g in (grads or (None, None, None))]
    ops.moe_gate_group_backward(ld, got[2], got[1], score, renormalize, scale, *gd, out=bufs[6][:T])
    torch.cuda.synchronize()
    if score == "sigmoid":                            # never written: still NaN
        assert bool(torch.isnan(bufs[2][:T]).all())
    res = [b[:n].cpu() for b, n in zip(bufs, rows)]
    if score == "sigmoid":
        res[2] = None
    return res, _guards_ok(bufs, rows)


def _check(logits, bias, want, ids_dtype, grads, what, exact=False):
    from mp4x.models.moe import gate_group_backward_torch, gate_group_forward_torch
    K, score, Gr, Kg, renormalize, scale = want.K, want.score, want.Gr, want.Kg, want.renormalize, want.scale
    # the float32 CPU evaluation is inside the bounds first
    cw, cids, clse, cps, _, cg = gate_group_forward_torch(logits, K, score, bias, Gr, Kg, renormalize, scale, torch.int64, True)
    assert want.selection_ok(cg, cids) is None, (what, "the float32 CPU evaluation", want.selection_ok(cg, cids))
    cgl = gate_group_backward_torch(logits, clse, cids, score, renormalize, scale, *grads)
    got, guards = _run(logits, bias, K, score, Gr, Kg, renormalize, scale, ids_dtype, grads)
    again, guards2 = _run(logits, bias, K, score, Gr, Kg, renormalize, scale, ids_dtype, grads)
    assert guards and guards2, (what, "guard rows")
    for a, b in zip(got, again):
        assert a is None or (same_bits(a, b) if a.is_floating_point() else torch.equal(a, b)), (what, "run to run")
    ids = got[1].to(torch.int64)
    assert got[1].dtype == ids_dtype and want.selection_ok(got[5], ids) is None, (what, want.selection_ok(got[5], ids))
    if exact:
        assert torch.equal(got[5].to(torch.int64), want.group_ids), (what, "group_ids")
        assert torch.equal(ids, want.ids), (what, "ids")
    assert torch.equal(got[4], torch.bincount(ids.reshape(-1), minlength=want.E)), (what, "counts")
    rows = [("weights", 0, cw, cids), ("prob_sum", 3, cps, None), ("g_logits", 6, cgl, cids)]
    if score == "softmax":
        rows.append(("lse", 2, clse, None))
    for name, i, cpu, cpu_ids in rows:
        for who, val, at in (("the float32 CPU evaluation", cpu, cpu_ids), ("K13", got[i], ids)):
            if name == "weights":
                w64, bound = want.weights(at)[0], want.weights_bound(at)
            elif name == "g_logits":
                w64, bound = want.backward(at, *grads)
            elif name == "lse":
                w64, bound = want.lse, want.lse_bound()
            else:
                w64, bound = want.prob_sum, want.prob_sum_bound()
            ok, ratio = ref.inside(val, w64, bound)
            if who == "K13":
                print(what, name, "worst / bound = %.3f" % ratio)
            assert ok, (what, name, who, ratio)


@pytest.mark.parametrize("shape", SHAPES)
def test_shapes_dtypes_and_bounds(shape):
    E, Gr, Kg, K = shape
    n, seen = 0, set()
    for ti, T in enumerate(TS):
        for score in ("sigmoid", "softmax"):
            # bias and renormalisation in all four combinations for every T and score; R and the scale
            # turn with T inside each combination, the dtype with the case count (3 and 4 are coprime)
            for ci, (with_bias, renormalize) in enumerate(((False, False), (True, True), (True, False), (False, True))):
                R, scale = (4, 32)[(ti + ci) % 2], (1.0, 2.5)[(ti + (ci >> 1)) % 2]
                for dtype in (DTYPES if E <= 8 else (DTYPES[n % 3],)):
                    which = ref.GRAD_SETS[1 + n % 7]              # every set of present gradients but the empty one
                    if score == "sigmoid":
                        which = (which[0], 0, which[2]) if (which[0] or which[2]) else (1, 0, 1)
                    logits, bias, want = ref.uniform_case(T, E, Gr, Kg, K, score, with_bias, renormalize, scale, R,
                                                          1000 + E + n, dtype)
                    assert (bias is not None) == with_bias
                    grads = ref.pick(ref.gradients(T, E, K, 2000 + E + n), which)
                    _check(logits, bias, want, (torch.int64, torch.int32)[n % 2], grads,
                           (T, shape, score, dtype, with_bias, renormalize, R))
                    seen |= {("R", score, with_bias, renormalize, R), ("dtype", score, with_bias, dtype), ("T", T, score, with_bias)}
                    n += 1
    # what ran, enumerated: every score with and without a bias and renormalisation at both spreads,
    # in every dtype and at every T
    assert len(seen) == 16 + 12 + 4 * len(TS), sorted(seen)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_separated_fixtures_give_exact_ids(dtype):
    for i, (kind, E, Gr, Kg, K, score, _) in enumerate(ref.SEPARATED):
        logits, bias, want = ref.separated_case(i, 65, dtype)
        grads = ref.gradients(65, E, K, 4000 + i)
        if score == "sigmoid":
            grads = (grads[0], None, grads[2])
        _check(logits, bias, want, (torch.int64, torch.int32)[i % 2], grads, (ref.SEPARATED[i], dtype), exact=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_bias_and_one_group_give_the_ids_of_k10(dtype):
    from mp4x.ops import device_ops as ops
    for E in (1, 2, 5, 8, 60, 64, 65, 128, 257, 2048):
        for n, K in enumerate(sorted({min(k, E) for k in (1, 2, 8, 16)})):
            logits, want = moe_gate_ref.cached_reference("ties", 65, E, K, True, 0, 500 + E, dtype)
            ld = logits.to(DEV)
            k10 = ops.moe_gate_topk(ld, K, True, stats=True)
            for score in ("softmax", "sigmoid"):
                got = ops.moe_gate_group_topk(ld, K, score, renormalize=True)
                assert torch.equal(got[1].cpu(), want.ids) and torch.equal(got[1], k10[1]), (E, K, score)
                assert bool((got[5] == 0).all())
            # the softmax score with nothing else is K10, bit for bit: the forward with its statistics ...
            got = ops.moe_gate_group_topk(ld, K, "softmax", renormalize=True, stats=True)
            assert same_bits(got[0].cpu(), k10[0].cpu()) and same_bits(got[2].cpu(), k10[2].cpu()), (E, K)
            assert same_bits(got[3].cpu(), k10[3].cpu()) and torch.equal(got[4], k10[4]), (E, K, "statistics")
            # ... and the backward of the same (logits, lse, ids) through either entry
            grads = moe_gate_ref.gradients(65, E, K, 600 + E)
            for renormalize in (False, True):
                for which in ((1, 1, 1), (1, 0, 0)):
                    gd = [None if g is None else g.to(DEV) for g in moe_gate_ref.pick(grads, which)]
                    g10 = ops.moe_gate_backward(ld, k10[2], k10[1], renormalize, *gd)
                    g13 = ops.moe_gate_group_backward(ld, k10[2], k10[1], "softmax", renormalize, 1.0, *gd)
                    assert same_bits(g13.cpu(), g10.cpu()), (E, K, renormalize, which)


def test_any_bits_give_ids_in_range_distinct_and_inside_the_chosen_groups():
    nan, inf = float("nan"), float("inf")
    for E, Gr, Kg, K in ((5, 1, 1, 5), (64, 1, 1, 8), (64, 8, 4, 8), (257, 1, 1, 16), (260, 4, 1, 16), (2048, 32, 8, 16),
                         (2048, 1, 1, 16)):
        lg = moe_gate_ref.uniform_logits(9, E, 4, 77)
        lg[0] = nan
        lg[1] = inf
        lg[2] = -inf
        lg[3, ::2] = nan
        lg[4, 1::3] = inf
        lg[5] = torch.tensor([0x7fffffff, -1, 0x7f800001, -8388607], dtype=torch.int32).view(torch.float32).repeat(E)[:E]
        lg[6, :E // 2] = -nan
        for n, dtype in enumerate(DTYPES):
            for score in ("sigmoid", "softmax"):
                for bias in (None, ref.random_bias(E, 5)):
                    ids_dtype = (torch.int64, torch.int32)[n % 2]
                    grads = ref.gradients(9, E, K, 78)
                    got, guards = _run(lg.to(getattr(torch, dtype)), bias, K, score, Gr, Kg, True, 2.5, ids_dtype,
                                       (grads[0], None, grads[2]) if score == "sigmoid" else grads)
                    ids, gids = got[1].to(torch.int64), got[5].to(torch.int64)
                    what = (E, Gr, dtype, score, bias is not None)
                    assert guards, what
                    assert bool(((ids >= 0) & (ids < E)).all()) and all(len(set(r)) == K for r in ids.tolist()), what
                    assert bool(((gids >= 0) & (gids < Gr)).all()) and all(len(set(r)) == Kg for r in gids.tolist()), what
                    assert bool(((ids // (E // Gr)).unsqueeze(2) == gids.unsqueeze(1)).any(dim=-1).all()), what
                    assert torch.equal(got[4], torch.bincount(ids.reshape(-1), minlength=E)), what
                    if Gr == 1 and bias is None:
                        # K10's order for any bits: every row, NaN and infinite ones included, against the
                        # K10 kernel (both order the same 32-bit keys); the ordinary rows against the sort
                        from mp4x.ops import device_ops as ops
                        k10 = ops.moe_gate_topk(lg.to(getattr(torch, dtype)).to(DEV), K, True, ids_dtype)[1]
                        assert torch.equal(got[1], k10.cpu()), what
                        assert torch.equal(ids[7:], moe_gate_ref.order_ids(lg.to(getattr(torch, dtype))[7:], K)), what


def test_no_token():
    from mp4x.ops import device_ops as ops
    lg = torch.empty(0, 8, device=DEV)
    w, ids, lse, ps, cnt, gids = ops.moe_gate_group_topk(lg, 3, "softmax", None, 4, 2, stats=True)
    assert w.shape == (0, 3) and ids.shape == (0, 3) and lse.shape == (0,) and gids.shape == (0, 2)
    assert ps.cpu().tolist() == [0.0] * 8 and cnt.cpu().tolist() == [0] * 8
    got = ops.moe_gate_group_topk(lg, 3, "sigmoid", None, 4, 2)
    assert got[2:5] == (None, None, None)
    assert ops.moe_gate_group_backward(lg, None, ids).shape == (0, 8)


def test_refusals_return_their_codes_without_a_launch():
    from mp4x.operators import DType
    from mp4x.ops import device_ops as ops, native
    lib = native.hip()
    T, E, K = 4, 8, 2
    lg = torch.zeros(T + 1, E, device=DEV)
    bias = torch.zeros(E + 1, device=DEV)
    bufs = [_guarded(T, (K,), torch.float32), _guarded(T, (K,), torch.int64), _guarded(T, (), torch.float32),
            _guarded(E, (), torch.float32), _guarded(E, (), torch.int64), _guarded(T, (2,), torch.int32),
            _guarded(T, (E,), torch.float32)]
    scratch = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    before = [b.clone() for b in bufs]

    def fwd(dtype=int(DType.F32), logits=lg.data_ptr(), b=bias.data_ptr(), T=T, E=E, K=K, Gr=4, Kg=2, score=1, scale=1.0,
            w=bufs[0].data_ptr(), ids=bufs[1].data_ptr(), gids=bufs[5].data_ptr(), lse=bufs[2].data_ptr(),
            ps=bufs[3].data_ptr(), cnt=bufs[4].data_ptr(), sc=scratch.data_ptr(), sb=1 << 16):
        return lib.mp4x_moe_gate_group_topk(dtype, logits, b, T, E, K, Gr, Kg, score, 0, scale, w, ids, 1, gids, lse, ps, cnt,
                                            sc, sb, None)

    def bwd(dtype=int(DType.F32), logits=lg.data_ptr(), T=T, E=E, K=K, score=1, scale=1.0, out=bufs[6].data_ptr(),
            ids=bufs[1].data_ptr(), lse=bufs[2].data_ptr()):
        return lib.mp4x_moe_gate_group_backward(dtype, logits, lse, ids, 1, T, E, K, score, 0, scale, None, None, None, out,
                                                None)

    bad, uns = native.E_BADARG, native.E_UNSUPPORTED
    for f in (fwd, bwd):
        assert [f(E=0), f(E=2049), f(K=0), f(K=17), f(E=8, K=9), f(T=-1)] == [bad] * 6
        assert [f(dtype=int(d)) for d in (DType.F64, DType.I32, DType.U8)] == [uns] * 3 and f(dtype=99) == uns
        assert f(logits=lg.data_ptr() + 4) == bad and f(logits=None) == bad and f(ids=bufs[1].data_ptr() + 4) == bad
        assert [f(score=2), f(score=-1)] == [uns] * 2
        assert [f(scale=0.0), f(scale=-1.0), f(scale=float("inf")), f(scale=float("nan"))] == [bad] * 4
        assert f(score=0, lse=None) == bad and f(lse=bufs[2].data_ptr() + 2) == bad
    assert [fwd(Gr=0), fwd(Gr=33), fwd(Gr=3), fwd(Gr=4, Kg=0), fwd(Gr=4, Kg=5), fwd(Gr=4, Kg=1, K=3)] == [bad] * 6
    assert fwd(E=64, Gr=64, Kg=4) == bad                                    # more than 32 groups
    assert fwd(w=bufs[0].data_ptr() + 2) == bad and fwd(b=bias.data_ptr() + 2) == bad and fwd(gids=bufs[5].data_ptr() + 2) == bad
    assert fwd(cnt=None) == bad and fwd(ps=None) == bad                      # the statistics: both or neither
    assert fwd(sc=scratch.data_ptr() + 16) == bad and fwd(sb=8) == bad and fwd(sc=None) == bad
    assert bwd(out=bufs[6].data_ptr() + 4) == bad and bwd(out=None) == bad
    assert lib.mp4x_moe_gate_group_scratch_bytes(int(DType.F64), 4, 8) == 0
    assert lib.mp4x_moe_gate_group_scratch_bytes(1, 4, 0) == 0
    torch.cuda.synchronize()
    assert all(same_bits(a, b) if a.is_floating_point() else torch.equal(a, b) for a, b in zip(bufs, before))
    # the wrappers refuse with the function's name
    b8 = torch.zeros(E, device=DEV)
    for call in (lambda: ops.moe_gate_group_topk(lg, 0), lambda: ops.moe_gate_group_topk(lg, 9),
                 lambda: ops.moe_gate_group_topk(lg.double(), 2), lambda: ops.moe_gate_group_topk(lg.cpu(), 2),
                 lambda: ops.moe_gate_group_topk(lg[:, :4], 2), lambda: ops.moe_gate_group_topk(lg, 2, ids_dtype=torch.int16),
                 lambda: ops.moe_gate_group_topk(lg, 2, "tanh"), lambda: ops.moe_gate_group_topk(lg, 2, n_group=3),
                 lambda: ops.moe_gate_group_topk(torch.zeros(2, 64, device=DEV), 2, n_group=64, topk_group=4),
                 lambda: ops.moe_gate_group_topk(lg, 2, n_group=4, topk_group=5),
                 lambda: ops.moe_gate_group_topk(lg, 3, n_group=4, topk_group=1),
                 lambda: ops.moe_gate_group_topk(lg, 2, scale=0.0), lambda: ops.moe_gate_group_topk(lg, 2, scale=float("nan")),
                 lambda: ops.moe_gate_group_topk(lg, 2, bias=b8[:7]), lambda: ops.moe_gate_group_topk(lg, 2, bias=b8.double()),
                 lambda: ops.moe_gate_group_topk(lg, 2, out=(bufs[0],) * 6)):
        with pytest.raises(ValueError, match="moe_gate_group_topk|device op"):
            call()
    ids = torch.zeros(T + 1, K, dtype=torch.int64, device=DEV)
    lse = torch.zeros(T + 1, device=DEV)
    for call in (lambda: ops.moe_gate_group_backward(lg, None, ids[:2]), lambda: ops.moe_gate_group_backward(lg, None, ids.float()),
                 lambda: ops.moe_gate_group_backward(lg, lse, ids), lambda: ops.moe_gate_group_backward(lg, None, ids, "softmax"),
                 lambda: ops.moe_gate_group_backward(lg, lse.double(), ids, "softmax"),
                 lambda: ops.moe_gate_group_backward(lg, None, ids, g_lse=lse),
                 lambda: ops.moe_gate_group_backward(lg, None, ids, scale=-2.0),
                 lambda: ops.moe_gate_group_backward(lg, None, ids, g_prob_sum=torch.zeros(E + 1, device=DEV)),
                 lambda: ops.moe_gate_group_backward(lg, None, ids, out=torch.zeros(T + 1, E, device=DEV, dtype=torch.float16))):
        with pytest.raises(ValueError, match="moe_gate_group_backward"):
            call()
