"""combineTokensBackward and ``combine_tokens(backward="fused")`` without a GPU: host tensors over
gloo run the torch form of K11's contract.  The expert rows' gradient has the bits of the dispatch
with ``row_scale`` (the parent's path), the weights' gradient is inside the bound of the float64
definition (tests/moe_combine_bwd_ref.py) and +0 on clipped assignments, along ragged, ``capacity=``
and ``sourceCapacity=`` plans; and the native refusals of the two K11 entry points on the real
libmp4x_hip.so (fake pointers: the checks are host-side and launch nothing)."""
import pytest

torch = pytest.importorskip("torch")

import moe_combine_bwd_ref as ref  # noqa: E402
from harness import run_ranks  # noqa: E402
from moe_ref import same_bits  # noqa: E402
from mp4x.operators import DType  # noqa: E402
from mp4x.ops import native  # noqa: E402

T, K, EL = 37, 3, 2
KINDS = {"ragged": {}, "capacity": {"capacity": 9}, "padded": {"sourceCapacity": 7}}
SHAPES = (("float32", 12), ("bfloat16", 24), ("float16", 8))


def _setup(comm, kind, dtype, width, seed):
    """One dispatch -> random expert outputs -> combine: everything the backward needs, on the host."""
    r, p = comm.getRank(), comm.getSlaveNum()
    E = EL * p
    dt = getattr(torch, dtype)
    x = ref.values(T, width, dt, seed + r)
    ids = ref.clipped_ids(T, K, E, seed + 10 + r)
    rows, plan = comm.dispatchTokens(x, ids, E, **KINDS[kind])
    y = ref.values(rows.numel() // width, width, dt, seed + 20 + r).view(rows.shape)
    w = ref.weights(T, K, seed + 30 + r)
    out, back = comm.combineTokens(y, plan, w, returnSlotRows=True)
    g = ref.values(T, width, dt, seed + 40 + r)
    return E, plan, y, w, back, g


def _api(comm):
    from mp4x import Mp4jException
    stats = comm.device.stats
    res = []
    for n, (kind, (dtype, width)) in enumerate((k, s) for k in KINDS for s in SHAPES):
        E, plan, y, w, back, g = _setup(comm, kind, dtype, width, 100 * n)
        want_rows = comm.device.dispatch_tokens(g, None, E, None, plan=plan, row_scale=w)[0]
        before = stats.get("moe.combine.backward", 0), stats.get("moe.dispatch", 0)
        g_rows, g_w = comm.combineTokensBackward(g, plan, w, back)
        again = comm.combine_tokens_backward(g, plan, w, back)
        counted = (stats.get("moe.combine.backward", 0) - before[0], stats.get("moe.dispatch", 0) - before[1])
        want64, bound = ref.definition(g, back, plan.slots, K)
        ok, ratio = ref.inside(g_w, want64, bound)
        refused = {}
        wrong = torch.zeros((back.shape[0] + 1,) + tuple(back.shape[1:]), dtype=back.dtype)
        for label, call in (("slotRows rows", lambda: comm.combineTokensBackward(g, plan, w, wrong)),
                            ("slotRows dtype", lambda: comm.combineTokensBackward(g, plan, w, back.to(torch.float64))),
                            ("no weights", lambda: comm.combineTokensBackward(g, plan, None, back)),
                            ("weights shape", lambda: comm.combineTokensBackward(g, plan, w[:-1], back)),
                            ("grad rows", lambda: comm.combineTokensBackward(g[:-1], plan, w, back)),
                            ("plan", lambda: comm.combineTokensBackward(g, (1, 2), w, back))):
            try:
                call()
                refused[label] = False
            except Mp4jException:
                refused[label] = True
        res.append(dict(what=(kind, dtype), rows=same_bits(g_rows, want_rows), shape=g_rows.shape == y.shape,
                        again=same_bits(again[0], want_rows) and same_bits(again[1], g_w), inside=ok, ratio=ratio,
                        zeros=ref.zero_bits_where_clipped(g_w, plan.slots), w_shape=g_w.shape == w.shape,
                        clipped=int((plan.slots < 0).sum()), live=int((plan.slots >= 0).sum()), counted=counted,
                        refused=refused))
    return res


@pytest.mark.parametrize("p", [1, 3])
def test_engine_api_on_host_tensors(p):
    res, code, errors = run_ranks(p, _api, timeout=120)
    assert sorted(res) == list(range(p)) and not errors and code == 0
    assert all(sum(res[r][i]["live"] for r in res) > 0 for i in range(len(KINDS) * len(SHAPES)))
    for r, rows in res.items():
        assert len(rows) == len(KINDS) * len(SHAPES)
        for row in rows:
            what = (r,) + row["what"]
            print(what, "worst / bound = %.3f" % row["ratio"])
            for key in ("rows", "shape", "again", "inside", "zeros", "w_shape"):
                assert row[key], (what, key, row["ratio"])
            assert row["clipped"] > K, (what, row["clipped"])                          # a whole token and more
            assert row["counted"] == (2, 0), (what, row["counted"])                    # never counted as a dispatch
            assert all(row["refused"].values()) and len(row["refused"]) == 6, (what, row["refused"])


def _autograd(comm):
    from mp4x.models.moe import combine_tokens
    res = []
    for n, kind in enumerate(KINDS):
        dtype, width = SHAPES[n]
        E, plan, y, w, back, g = _setup(comm, kind, dtype, width, 1000 + 100 * n)
        grads = {}
        for how in ("torch", "fused"):
            yd, wd = y.clone().requires_grad_(True), w.clone().requires_grad_(True)
            before = comm.device.stats.get("moe.combine.backward", 0)
            combine_tokens(comm, yd, plan, wd, backward=how).backward(g)
            grads[how] = (yd.grad, wd.grad, comm.device.stats.get("moe.combine.backward", 0) - before)
        yd = y.clone().requires_grad_(True)
        combine_tokens(comm, yd, plan, None, backward="fused").backward(g)           # no weights: the existing path
        want_unit = comm.device.dispatch_tokens(g, None, E, None, plan=plan)[0]
        want64, bound = ref.definition(g, back, plan.slots, K)
        res.append(dict(what=(kind, dtype), rows=same_bits(grads["fused"][0], grads["torch"][0]),
                        torch=ref.inside(grads["torch"][1], want64, bound), fused=ref.inside(grads["fused"][1], want64, bound),
                        zeros=ref.zero_bits_where_clipped(grads["fused"][1], plan.slots),
                        counted=(grads["torch"][2], grads["fused"][2]), unit=same_bits(yd.grad, want_unit)))
    return res


@pytest.mark.parametrize("p", [1, 2])
def test_autograd_fused_against_torch(p):
    res, code, errors = run_ranks(p, _autograd, timeout=120)
    assert sorted(res) == list(range(p)) and not errors and code == 0
    for r, rows in res.items():
        assert len(rows) == len(KINDS)
        for row in rows:
            what = (r,) + row["what"]
            assert row["rows"] and row["zeros"] and row["unit"], (what, row)
            assert row["torch"][0] and row["fused"][0], (what, row["torch"], row["fused"])
            assert row["counted"] == (0, 1), (what, row["counted"])


def test_unknown_values_raise():
    from mp4x.models.moe import ExpertParallelMoE, combine_tokens
    with pytest.raises(ValueError, match="backward"):
        combine_tokens(None, torch.zeros(2, 4), None, None, backward="hip")
    with pytest.raises(ValueError, match="combine_backward"):
        ExpertParallelMoE(None, 4, 8, 2, 1, combine_backward="kernel")


def test_the_definition_and_its_bound_on_a_cancelling_case():
    """rows = +-g alternating: the exact dot product is 0 while sum |g * y| is not, and the float32
    evaluation of it is inside a bound on sum |.|, not on the value."""
    g, rows, slots = ref.cancelling(5, 64, torch.float32, 7)
    want64, bound = ref.definition(g, rows, slots, 2)
    assert bool((want64[:, 0] == 0).all()) and bool((bound > 0).all()) and bool((want64[:, 1] > 0).all())
    assert ref.inside(ref.torch_f32(g, rows, slots, 2), want64, bound)[0]
    assert not ref.inside(want64 + 2 * bound, want64, bound)[0]


# ---------------------------------------------------------------- the native refusals
BADARG, UNSUPPORTED = 1001, 1002
G, ROWS, G_ROWS, SLOTS, W, G_W, SCRATCH = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000


def _lib():
    try:
        return native.hip()
    except Exception as e:   # noqa: BLE001
        pytest.skip(f"libmp4x_hip.so not loadable: {e}")


def _bwd(lib, dtype=DType.F32, g=G, rows=ROWS, num_rows=519, slots=SLOTS, w=W, T=173, K=3, width=4, g_rows=G_ROWS,
         g_w=G_W):
    return lib.mp4x_moe_combine_backward(int(dtype), g, rows, num_rows, slots, w, T, K, width, g_rows, g_w, None)


def _bwd_pad(lib, dtype=DType.F32, g=G, rows=ROWS, slots=SLOTS, w=W, T=173, K=3, width=4, n=519, nb=8, cap=70,
             scratch=SCRATCH, sb=None, g_rows=G_ROWS, g_w=G_W):
    sb = lib.mp4x_moe_route_scratch_bytes(n, nb) if sb is None else sb
    return lib.mp4x_moe_combine_backward_pad(int(dtype), g, rows, slots, w, T, K, width, n, nb, cap, scratch, sb,
                                             g_rows, g_w, None)


COMMON = [
    (dict(dtype=DType.F64), UNSUPPORTED), (dict(dtype=DType.I32), UNSUPPORTED), (dict(dtype=99), UNSUPPORTED),
    (dict(T=-1), BADARG), (dict(K=0), BADARG), (dict(K=17), BADARG), (dict(width=0), BADARG), (dict(width=6), BADARG),
    (dict(dtype=DType.BF16, width=4), BADARG),                # a row of 8 bytes
    (dict(g=None), BADARG), (dict(g=G + 8), BADARG), (dict(rows=None), BADARG), (dict(rows=ROWS + 4), BADARG),
    (dict(g_rows=None), BADARG), (dict(g_rows=G_ROWS + 8), BADARG), (dict(slots=None), BADARG),
    (dict(slots=SLOTS + 4), BADARG), (dict(w=None), BADARG), (dict(w=W + 2), BADARG), (dict(g_w=None), BADARG),
    (dict(g_w=G_W + 2), BADARG),
    (dict(g_rows=ROWS), BADARG), (dict(g_rows=ROWS + 16), BADARG), (dict(g_rows=G), BADARG),    # aliasing
    (dict(g_rows=G + 173 * 16 - 16), BADARG),
]


@pytest.mark.parametrize("case,want", COMMON + [(dict(num_rows=0), BADARG), (dict(T=1 << 30, K=2), BADARG),
                                                (dict(rows=G_ROWS + 519 * 16 - 16), BADARG)])
def test_combine_backward_refuses_without_launching(case, want):
    assert _bwd(_lib(), **case) == want


@pytest.mark.parametrize("case,want", COMMON + [
    (dict(n=520), BADARG), (dict(nb=0), BADARG), (dict(nb=2049), BADARG), (dict(cap=0), BADARG),
    (dict(cap=1 << 31), BADARG), (dict(scratch=None), BADARG), (dict(scratch=SCRATCH + 16), BADARG), (dict(sb=64), BADARG),
    (dict(rows=G_ROWS + 560 * 16 - 16), BADARG),              # the padded buffer is nb * cap rows long
])
def test_combine_backward_pad_refuses_without_launching(case, want):
    assert _bwd_pad(_lib(), **case) == want


def test_the_empty_call_launches_nothing():
    assert _bwd(_lib(), T=0, g=None, rows=None, slots=None, w=None, g_rows=None, g_w=None) == 0
