"""The gated (SwiGLU) expert activation on host tensors: the torch forms ``glu_torch`` /
``glu_backward_torch`` (the definition a kernel has to implement, and the CPU form) against the
float64 definition of tests/moe_glu_ref.py inside the derived bounds; torch's
own autograd of ``silu(gate) * up`` inside the same bounds; rows nobody owns poisoned with NaN and
still +0 in every output; every refusal; and the edge fixture.  No GPU."""
import pytest

torch = pytest.importorskip("torch")

import moe_glu_ref as ref  # noqa: E402
from moe_glu_ref import same_bits  # noqa: E402

NS = (1, 7, 8, 24)
SCALES = (1.0, 4.0, 16.0)


def _cases():
    n = 0
    for name, (table, R, segs) in ref.tables().items():
        for dtype in ref.DTYPES:
            for N in NS:
                scale = SCALES[n % 3]
                n += 1
                yield name, table, R, segs, N, dtype, scale, 100 + n


def _worst(rows):
    worst = {}
    for what, ok, ratio in rows:
        assert ok, (what, ratio)
        key = what[0] + " " + str(what[3]).replace("torch.", "")
        worst[key] = max(worst.get(key, 0.0), ratio)
    return worst


def test_the_torch_forms_are_inside_the_bounds():
    from mp4x.parallel.moe import glu_backward_torch, glu_torch
    rows, scales = [], set()
    for name, table, R, segs, N, dtype, scale, seed in _cases():
        pre, g_h, own = ref.case(table, R, segs, N, dtype, scale, seed)
        scales.add((dtype, scale))
        h64, hb = ref.forward64(pre, own)
        g64, gb = ref.backward64(pre, g_h, own)
        h, gp = glu_torch(pre, table), glu_backward_torch(pre, g_h, table)
        assert h.shape == pre.shape[:-1] + (N,) and gp.shape == pre.shape and h.dtype == gp.dtype == dtype
        # a row nobody owns held NaN in pre and g_h: +0 bits in both outputs
        dead = ~own
        assert same_bits(h.reshape(R, N)[dead], torch.zeros(int(dead.sum()), N, dtype=dtype)), (name, N, dtype)
        assert same_bits(gp.reshape(R, 2 * N)[dead], torch.zeros(int(dead.sum()), 2 * N, dtype=dtype)), (name, N, dtype)
        rows.append((("h", name, N, dtype), *ref.inside(h, h64, hb, dtype)))
        rows.append((("g_gate", name, N, dtype), *ref.inside(gp.reshape(R, 2 * N)[:, :N], g64[:, :N], gb[:, :N], dtype)))
        rows.append((("g_up", name, N, dtype), *ref.inside(gp.reshape(R, 2 * N)[:, N:], g64[:, N:], gb[:, N:], dtype)))
    assert len(scales) == 9, sorted(scales, key=str)            # every dtype at every scale
    worst = _worst(rows)
    print("the torch forms: worst / bound =", {k: round(v, 3) for k, v in worst.items()})
    assert all(v < 1.0 for v in worst.values()), worst


def test_torch_autograd_of_silu_times_up_is_inside_the_same_bounds():
    rows = []
    for name, table, R, segs, N, dtype, scale, seed in _cases():
        pre, g_h, own = ref.case(table, R, segs, N, dtype, scale, seed)
        if not bool(own.any()):
            continue
        h64, hb = ref.forward64(pre, own)
        g64, gb = ref.backward64(pre, g_h, own)
        # float32 on the owned rows, as a user writes it; one rounding at the end
        x = pre.reshape(R, 2 * N)[own].to(torch.float32).requires_grad_(True)
        h = torch.nn.functional.silu(x[:, :N]) * x[:, N:]
        h.backward(g_h.reshape(R, N)[own].to(torch.float32))
        rows.append((("h", name, N, dtype), *ref.inside(h.detach().to(dtype), h64[own], hb[own], dtype)))
        g = x.grad.to(dtype)
        rows.append((("g_gate", name, N, dtype), *ref.inside(g[:, :N], g64[own][:, :N], gb[own][:, :N], dtype)))
        rows.append((("g_up", name, N, dtype), *ref.inside(g[:, N:], g64[own][:, N:], gb[own][:, N:], dtype)))
    worst = _worst(rows)
    print("torch autograd: worst / bound =", {k: round(v, 3) for k, v in worst.items()})
    assert all(v < 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_the_edge_fixture(dtype):
    from mp4x.parallel.moe import glu_backward_torch, glu_torch
    pre, g_h, table = ref.edge_case(dtype)
    assert ref.edge_check(glu_torch(pre, table), pre) is None, ref.edge_check(glu_torch(pre, table), pre)
    gp = glu_backward_torch(pre, g_h, table)
    assert ref.edge_check(gp, pre, g_h) is None, ref.edge_check(gp, pre, g_h)
    # torch's own silu has the same classes, its NaN at g = -inf included
    own = torch.nn.functional.silu(pre[:, :ref.EDGE_N].to(torch.float32)) * pre[:, ref.EDGE_N:].to(torch.float32)
    assert torch.equal(ref.classes(own.to(dtype)), ref.classes(glu_torch(pre, table)))


def test_every_refusal_names_its_argument():
    from mp4x.parallel.moe import glu_backward_torch, glu_torch
    rt = ("ragged", torch.tensor([0, 4], dtype=torch.int64))
    pt = ("padded", torch.tensor([[1, 2]], dtype=torch.int64), 2)
    pre, gh = torch.zeros(4, 6), torch.zeros(4, 3)
    pp = torch.zeros(1, 4, 6)
    bad_fwd = [
        (dict(pre=pre.double(), table=rt), "pre"),                                   # a dtype outside the three
        (dict(pre=pre.to(torch.int32), table=rt), "pre"),
        (dict(pre=torch.zeros(4, 12)[:, ::2], table=rt), "pre"),                     # not contiguous
        (dict(pre=torch.zeros(4, 5), table=rt), "pre"),                              # an odd last dimension
        (dict(pre=torch.zeros(6), table=rt), "pre"),
        (dict(pre=pp, table=rt), "pre"),                                             # a shape that does not fit the table
        (dict(pre=pre, table=pt), "pre"),
        (dict(pre=torch.zeros(1, 6, 6), table=pt), "pre"),
        (dict(pre=torch.zeros(2, 4, 6), table=pt), "pre"),
        (dict(pre=pre, table=("ragged", torch.tensor([0, 4], dtype=torch.int32))), "table"),      # another dtype
        (dict(pre=pre, table=("ragged", torch.tensor([0, 4], dtype=torch.int64, device="meta"))), "table"),
        (dict(pre=pre, table=("ragged", torch.zeros(1, 2, dtype=torch.int64))), "table|ragged"),
        (dict(pre=pre, table=("ragged",)), "table"),
        (dict(pre=pre, table=("blocked", rt[1])), "table"),
        (dict(pre=pre, table=[rt[0], rt[1]]), "table"),
        (dict(pre=pp, table=("padded", pt[1], 0)), "S"),                             # S < 1
        (dict(pre=pp, table=("padded", pt[1], True)), "S"),
        (dict(pre=pp, table=("padded", pt[1], 2.0)), "S"),
        (dict(pre=pp, table=("padded", pt[1])), "table|padded"),
    ]
    for kw, match in bad_fwd:
        with pytest.raises(ValueError, match=match):
            glu_torch(kw["pre"], kw["table"])
        with pytest.raises(ValueError, match=match):
            glu_backward_torch(kw["pre"], torch.zeros(kw["pre"].shape[:-1] + (kw["pre"].shape[-1] // 2,)), kw["table"])
    for g in (gh.double(), torch.zeros(4, 6)[:, ::2], torch.zeros(4, 4), torch.zeros(3, 3), gh.to(torch.bfloat16)):
        with pytest.raises(ValueError, match="g_h"):
            glu_backward_torch(pre, g, rt)
    # no row and no column are not refused
    assert glu_torch(torch.zeros(0, 6), ("ragged", torch.tensor([0, 0], dtype=torch.int64))).shape == (0, 3)
    assert glu_torch(torch.zeros(4, 0), rt).shape == (4, 0)
    assert glu_backward_torch(torch.zeros(4, 0), torch.zeros(4, 0), rt).shape == (4, 0)
