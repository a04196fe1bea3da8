"""Float edge cases of the reducers on the device: NaN, infinities and signed zeros through K1
(reduce_, reduce_strided_), the three reduce-by-key paths and scale_, and the 16-bit float and
uint8 rows of K1 — against a sequential CPU loop in the accumulator type.

The rule of MAX / MIN is written out here, not copied from csrc/kernels/common.hpp: a NaN in the
accumulated value wins, else a NaN in the incoming value wins, else >= / <=.  NaN POSITIONS are
compared (payloads differ between an x86 and a GPU NaN, and after a bf16 / f16 store), everything
else bit for bit.  A MAX / MIN tie between +0 and -0 compares as equal: the sign of a zero tie is
not part of the contract."""
import pytest

torch = pytest.importorskip("torch")

from mp4x.operators import OpCode  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
FLOATS = [torch.float32, torch.float64, torch.bfloat16, torch.float16]
ARITH = [OpCode.SUM, OpCode.PROD, OpCode.MAX, OpCode.MIN]
_IVIEW = {torch.float32: torch.int32, torch.float64: torch.int64, torch.bfloat16: torch.int16,
          torch.float16: torch.int16}
_SPECIALS = [float("nan"), float("inf"), float("-inf"), 0.0, -0.0, None]     # None: keep the random value
_ids = lambda v: str(v).replace("torch.", "").replace("OpCode.", "")  # noqa: E731
N = 9247      # every element width: full tiles, a partial tile, whole vectors past it, a scalar tail


def _K():
    from mp4x.ops import device_ops, native
    native.hip()
    return device_ops


def _acc_t(dtype):
    return torch.float32 if dtype in (torch.bfloat16, torch.float16) else dtype


def _combine(a, b, op):
    if op == OpCode.SUM:
        return a + b
    if op == OpCode.PROD:
        return a * b
    pick = (a >= b) if op == OpCode.MAX else (a <= b)
    return torch.where(torch.isnan(a), a, torch.where(torch.isnan(b), b, torch.where(pick, a, b)))


def _ref_chain(xs, op, dtype):
    """Sequential, in input order, in the accumulator type, stored once per launch: a launch takes
    8 inputs, and every further launch the stored result and 7 more — so 16-bit floats round after
    inputs 8, 15, 22, ... as well as at the end (f32 / f64: the store is exact)."""
    at = _acc_t(dtype)
    acc = xs[0].to(at)
    in_launch = 1
    for x in xs[1:]:
        if in_launch == 8:
            acc = acc.to(dtype).to(at)
            in_launch = 1
        acc = _combine(acc, x.to(at), op)
        in_launch += 1
    return acc.to(dtype)


def _same(got, ref, op=None):
    got, ref = got.detach().cpu().contiguous(), ref.detach().cpu().contiguous()
    assert got.dtype == ref.dtype and got.shape == ref.shape
    gn, rn = torch.isnan(got), torch.isnan(ref)
    diff = got.view(_IVIEW[got.dtype]) != ref.view(_IVIEW[ref.dtype])
    if op in (OpCode.MAX, OpCode.MIN):
        diff &= ~((got == 0) & (ref == 0))                     # a +0 / -0 tie is not pinned
    bad = (gn != rn) | (~rn & diff)
    assert not bad.any(), (int(bad.sum()), bad.nonzero()[:8].tolist())


def _planted(shape, nin, dtype, seed, every=7):
    """nin random tensors; the first, a middle and the last get NaN, +Inf, -Inf, +0, -0 (or keep
    their value) at every `every`-th element and at the last 8, cycling so that all combinations
    across the three inputs occur (Inf - Inf, 0 * Inf, NaN against everything, +0 against -0)."""
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn(shape, generator=g).clamp(-1.5, 1.5).to(dtype) for _ in range(nin)]
    n = xs[0].numel()
    pos = torch.unique(torch.cat([torch.arange(0, n, every), torch.arange(max(n - 8, 0), n)]))
    order = torch.arange(pos.numel())
    for j, k in enumerate(sorted({0, nin // 2, nin - 1})):
        digit = (order // (6 ** j)) % 6
        flat = xs[k].view(-1)
        for d, v in enumerate(_SPECIALS):
            if v is not None:
                flat[pos[digit == d]] = v
    return xs


# ---------------------------------------------------------------- K1
@pytest.mark.parametrize("dtype", FLOATS, ids=_ids)
@pytest.mark.parametrize("op", ARITH, ids=_ids)
@pytest.mark.parametrize("nin", [2, 3, 8, 11])
def test_reduce_float_edges(dtype, op, nin):
    """The 16-byte tile kernel (aligned operands), the scalar kernel (operands one element off
    16-byte alignment) and the in-place form."""
    K = _K()
    xs = _planted((N,), nin, dtype, seed=nin * 10 + int(op))
    ref = _ref_chain(xs, op, dtype)
    assert torch.isnan(ref).any() and torch.isinf(ref).any()
    dx = [x.to(DEV) for x in xs]
    out = torch.empty(N, dtype=dtype, device=DEV)
    K.reduce_(out, dx, int(op))
    _same(out, ref, op)
    mis = [torch.cat([x[:1], x]).to(DEV)[1:] for x in xs]
    assert all(m.data_ptr() % 16 for m in mis)
    out2 = torch.empty(N + 1, dtype=dtype, device=DEV)[1:]
    K.reduce_(out2, mis, int(op))
    _same(out2, ref, op)
    acc = dx[0].clone()
    K.reduce_(acc, [acc] + dx[1:], int(op))
    _same(acc, ref, op)


_U8_OPS = [OpCode.SUM, OpCode.MAX, OpCode.MIN, OpCode.PROD, OpCode.BAND, OpCode.BOR, OpCode.BXOR]


@pytest.mark.parametrize("op", _U8_OPS, ids=_ids)
@pytest.mark.parametrize("nin", [2, 3, 8, 11])
def test_reduce_uint8(op, nin):
    """uint8 over its whole range: SUM and PROD wrap modulo 256, MAX / MIN are unsigned."""
    K = _K()
    g = torch.Generator().manual_seed(nin * 10 + int(op))
    xs = [torch.randint(0, 256, (N,), generator=g, dtype=torch.int64) for _ in range(nin)]
    if op == OpCode.PROD:                                       # odd factors: the product never dies to 0
        xs = [x | 1 for x in xs]
    acc = xs[0].clone()
    for x in xs[1:]:
        acc = {OpCode.SUM: lambda: (acc + x) & 0xFF, OpCode.PROD: lambda: (acc * x) & 0xFF,
               OpCode.MAX: lambda: torch.maximum(acc, x), OpCode.MIN: lambda: torch.minimum(acc, x),
               OpCode.BAND: lambda: acc & x, OpCode.BOR: lambda: acc | x, OpCode.BXOR: lambda: acc ^ x}[op]()
    ref = acc.to(torch.uint8)
    dx = [x.to(torch.uint8).to(DEV) for x in xs]
    out = torch.empty(N, dtype=torch.uint8, device=DEV)
    K.reduce_(out, dx, int(op))
    assert torch.equal(out.cpu(), ref)
    mis = [torch.cat([x[:1], x]).to(torch.uint8).to(DEV)[1:] for x in xs]
    out2 = torch.empty(N + 1, dtype=torch.uint8, device=DEV)[1:]
    K.reduce_(out2, mis, int(op))
    assert torch.equal(out2.cpu(), ref)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_ids)
@pytest.mark.parametrize("op", [OpCode.SUM, OpCode.MAX], ids=_ids)
@pytest.mark.parametrize("nin", [1, 8, 9, 64])
@pytest.mark.parametrize("n", [N, N + 1])
def test_reduce_strided(dtype, op, nin, n):
    """reduce_strided_ over nin chunks laid out back to back == reduce_ of the same slices (odd n:
    the chunks lose their 16-byte alignment), and == the CPU loop."""
    K = _K()
    xs = _planted((n,), nin, dtype, seed=nin + n)
    base = torch.cat(xs).to(DEV)
    out = torch.empty(n, dtype=dtype, device=DEV)
    K.reduce_strided_(out, base, nin, int(op))
    want = torch.empty(n, dtype=dtype, device=DEV)
    K.reduce_(want, [base[k * n:(k + 1) * n] for k in range(nin)], int(op))
    assert torch.equal(out.view(_IVIEW[dtype]), want.view(_IVIEW[dtype]))
    _same(out, _ref_chain(xs, op, dtype), op)


# ---------------------------------------------------------------- reduce-by-key
def _rbk_ref(keys, vals, op):
    """Every key's rows combined in input order in the accumulator type, rounded once."""
    at = _acc_t(vals.dtype)
    v = vals.to(at)
    acc, cnt = {}, {}
    for i, k in enumerate(keys.tolist()):
        acc[k] = _combine(acc[k], v[i], op) if k in acc else v[i].clone()
        cnt[k] = cnt.get(k, 0) + 1
    uk = sorted(acc)
    return (torch.tensor(uk, dtype=torch.int64), torch.stack([acc[k] for k in uk]).to(vals.dtype),
            torch.tensor([cnt[k] for k in uk], dtype=torch.int32))


@pytest.mark.parametrize("dtype", FLOATS, ids=_ids)
@pytest.mark.parametrize("op", ARITH, ids=_ids)
def test_reduce_by_key_float_edges(dtype, op):
    """The sort, hash and dense paths with the planted values, rows of 16 bytes (vector kernels)
    and of 3 elements (scalar kernels); 300 rows over 41 keys keeps the hash runs in list order."""
    K = _K()
    n = 300
    g = torch.Generator().manual_seed(17)
    keys = torch.randint(0, 41, (n,), generator=g, dtype=torch.int64)
    assert int(torch.bincount(keys).max()) <= 64
    for dim in (16 // torch.empty(0, dtype=dtype).element_size(), 3):
        vals = _planted((n, dim), 1, dtype, seed=int(op) + dim, every=3)[0]
        ref_k, ref_v, ref_c = _rbk_ref(keys, vals, op)
        assert torch.isnan(ref_v).any()
        dk, dv = keys.to(DEV), vals.to(DEV)

        def same(got, path):
            uk, uv, cnt = got
            assert torch.equal(uk.cpu(), ref_k), (path, dim)
            assert torch.equal(cnt.cpu(), ref_c), (path, dim)
            _same(uv.reshape(ref_v.shape), ref_v, op)

        same(K.reduce_by_key(dk, dv, int(op)), "sort")
        hk, hv, hc = K.hash_reduce_by_key(dk, dv, int(op))
        order = torch.argsort(hk)
        same((hk[order], hv[order], hc[order]), "hash")
        dense = K.dense_reduce_by_key(dk, dv, int(op), 0, 1, 64)
        assert dense is not None
        same(dense, "dense")


# ---------------------------------------------------------------- scale
@pytest.mark.parametrize("dtype", FLOATS, ids=_ids)
@pytest.mark.parametrize("s", [1.0 / 3.0, 1.0 / 7.0], ids=["third", "seventh"])
@pytest.mark.parametrize("off", [0, 1])
def test_scale_inexact_factor(dtype, s, off):
    """Factors that are exact in no dtype: the product is taken in the accumulator type (f32 for
    the 16-bit floats, the factor rounded to it once; a plain double multiply for f64) and stored
    with one rounding.  The vector form (aligned), the scalar form (one element off), in place."""
    K = _K()
    n = 12345
    x = _planted((n + off,), 1, dtype, seed=off + 3)[0]
    at = _acc_t(dtype)
    ref = (x.to(at) * torch.tensor(s, dtype=at)).to(dtype)[off:]
    dx = x.to(DEV)[off:]
    y = torch.empty(n + off, dtype=dtype, device=DEV)[off:]
    K.scale_(y, dx, s)
    _same(y, ref)
    z = dx.clone()
    K.scale_(z, z, s)
    _same(z, ref)
