"""The codec reference of tests/fp8_ref.py checked against first principles on the CPU: the GPU
tests compare the kernels with it bit for bit, so it has to be right on its own, and the
comparison has to have teeth (a plausible wrong codec must differ from it)."""
import pytest

torch = pytest.importorskip("torch")

from fp8_ref import QBLOCK, decode, ref_dequant_reduce, ref_quant, ref_store  # noqa: E402


def _code_value(c: int) -> float:
    """e4m3fn by its definition: 1 sign, 4 exponent (bias 7), 3 mantissa bits; no infinities,
    S.1111.111 is NaN."""
    s = -1.0 if c & 0x80 else 1.0
    e, m = (c >> 3) & 0xF, c & 7
    if e == 15 and m == 7:
        return float("nan")
    if e == 0:
        return s * m / 8.0 * 2.0 ** -6
    return s * (1 + m / 8.0) * 2.0 ** (e - 7)


def _data(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g) * torch.logspace(-3, 3, n)


def test_all_256_codes_round_trip():
    codes = torch.arange(256, dtype=torch.int64).to(torch.uint8)
    vals = decode(codes)
    for c in range(256):
        want = _code_value(c)
        got = float(vals[c])
        assert (got != got) if want != want else (got == want), c
    assert float(vals[0x80]) == 0.0 and torch.signbit(vals[0x80])
    back = vals.to(torch.float8_e4m3fn).view(torch.uint8)
    nan = torch.isnan(vals)
    assert torch.equal(back[~nan], codes[~nan])
    assert nan.nonzero().view(-1).tolist() == [0x7F, 0xFF]
    assert all(int(b) & 0x7F == 0x7F for b in back[nan])
    # a block that holds every finite code's value and +-448 has scale 1: the codes come back
    blk = torch.zeros(QBLOCK)
    blk[:254] = vals[~nan]
    q, s = ref_quant(blk)
    assert float(s[0]) == 1.0
    assert torch.equal(q[:254], codes[~nan])


def test_ties_round_to_nearest_even_and_nan_is_0x7f():
    # in [16, 32) the e4m3 spacing is 2: 17 and 19 are ties; 2^-10 is half of the smallest
    # subnormal 2^-9 and ties to the even code 0
    x = torch.tensor([17.0, 19.0, 2.0 ** -10, -17.0, -19.0, 3 * 2.0 ** -10, float("nan")])
    q = x.to(torch.float8_e4m3fn)
    assert q.float()[:6].tolist() == [16.0, 20.0, 0.0, -16.0, -20.0, 2.0 ** -8]
    assert int(q.view(torch.uint8)[6]) == 0x7F
    blk = torch.zeros(QBLOCK)
    blk[:7] = x
    blk[7] = 448.0                                            # scale 1
    qq, s = ref_quant(blk)
    assert float(s[0]) == 1.0
    assert decode(qq)[:6].tolist() == [16.0, 20.0, 0.0, -16.0, -20.0, 2.0 ** -8]
    assert int(qq[6]) == 0x7F and int(qq[7]) == 0x7E


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_amax_element_encodes_to_the_largest_code(dtype):
    n = QBLOCK * 40 + 100
    x = _data(n, 3).to(dtype)
    q, s = ref_quant(x)
    assert q.numel() == 41 * QBLOCK and s.numel() == 41 and s.dtype == torch.float32
    xf = torch.zeros(41 * QBLOCK)
    xf[:n] = x.float()
    b = xf.view(41, QBLOCK)
    j = b.abs().argmax(dim=1)
    top = q.view(41, QBLOCK)[torch.arange(41), j]
    neg = b[torch.arange(41), j] < 0
    assert torch.equal(top, torch.where(neg, torch.tensor(0xFE), torch.tensor(0x7E)).to(torch.uint8))
    assert neg.any() and (~neg).any()
    assert torch.equal(s, b.abs().amax(1) / 448.0)
    assert not q[n:].any()                                     # the pad encodes to 0x00
    # the decoded value is within half an e4m3 step of the input: 2^-4 relative for normal codes
    # (|code| >= 2^-6), half of the subnormal step 2^-9 below; 1e-6 covers the f32 roundings of
    # scale, 1 / scale and the products
    code = decode(q).view(41, QBLOCK)
    y = code * s[:, None]
    bound = (torch.maximum(code.abs() * 2.0 ** -4, torch.tensor(2.0 ** -10)) * s[:, None]) * (1 + 1e-6)
    assert ((y - b).abs() <= bound).all()


def test_zero_block_and_negative_zero():
    x = torch.zeros(2 * QBLOCK)
    x[5] = -0.0
    x[QBLOCK + 7] = -0.0
    x[QBLOCK + 9] = 3.0
    q, s = ref_quant(x)
    assert float(s[0]) == 1.0 and float(s[1]) == float(torch.tensor(3.0) / 448.0)
    assert int(q[5]) == 0x80 and int(q[QBLOCK + 7]) == 0x80 and int(q[QBLOCK + 9]) == 0x7E
    q[5] = 0
    q[QBLOCK + 7] = 0
    q[QBLOCK + 9] = 0
    assert not q.any()


def test_nan_and_inf_blocks():
    x = _data(3 * QBLOCK, 5)
    y = x.clone()
    y[10] = float("nan")
    y[QBLOCK + 3] = float("inf")
    q0, s0 = ref_quant(x)
    x_wo = x.clone()
    x_wo[10] = 0.0
    q1, s1 = ref_quant(x_wo)
    q, s = ref_quant(y)
    # the NaN is ignored in the amax and encodes to NaN; the rest of its block is unchanged
    assert int(q[10]) == 0x7F
    keep = torch.ones(QBLOCK, dtype=torch.bool)
    keep[10] = False
    assert torch.equal(q[:QBLOCK][keep], q1[:QBLOCK][keep]) and float(s[0]) == float(s1[0])
    # the Inf block: infinite scale, nothing in it decodes to a finite value
    assert float(s[1]) == float("inf")
    acc, amb = ref_dequant_reduce([q], [s])
    assert amb == 0
    assert not torch.isfinite(acc[QBLOCK:2 * QBLOCK]).any()
    assert torch.isnan(acc[10]) and torch.isfinite(acc[:QBLOCK][keep]).all()
    # the finite block next to them is untouched
    assert torch.equal(q[2 * QBLOCK:], q0[2 * QBLOCK:]) and float(s[2]) == float(s0[2])


def _quantised(nin, n, seed):
    qs, ss = zip(*[ref_quant(_data(n, seed * 100 + k)) for k in range(nin)])
    return list(qs), list(ss)


def test_chain_is_an_fma_chain_and_the_comparison_has_teeth():
    n = QBLOCK * 6
    qs, ss = _quantised(8, n, 1)
    acc, amb = ref_dequant_reduce(qs, ss)
    assert amb == 0
    # fan-in 1 from zero: the product rounded once
    a1, amb1 = ref_dequant_reduce(qs[:1], ss[:1])
    assert amb1 == 0
    assert torch.equal(a1, decode(qs[0]) * ss[0].repeat_interleave(QBLOCK))
    # the float64 sum of the products agrees to an f32 ulp of the terms per step
    ex = sum(decode(q).double() * s.double().repeat_interleave(QBLOCK) for q, s in zip(qs, ss))
    assert ((acc.double() - ex).abs() <= 8 * 2.0 ** -23 * sum(
        (decode(q).double() * s.double().repeat_interleave(QBLOCK)).abs() for q, s in zip(qs, ss))).all()
    # mul then add in f32 (two roundings per step) is a different function
    plain = torch.zeros(n)
    for q, s in zip(qs, ss):
        plain = plain + decode(q) * s.repeat_interleave(QBLOCK)
    assert int((plain.view(torch.int32) != acc.view(torch.int32)).sum()) > n // 10
    # accumulate continues the chain: 3 then 5 more == 8
    head, a_amb = ref_dequant_reduce(qs[:3], ss[:3])
    tail, b_amb = ref_dequant_reduce(qs[3:], ss[3:], acc0=head)
    assert a_amb == 0 and b_amb == 0
    assert torch.equal(tail.view(torch.int32), acc.view(torch.int32))
    # the order of the inputs matters
    rev, _ = ref_dequant_reduce(qs[::-1], ss[::-1])
    assert not torch.equal(rev, acc)


def test_ambiguous_steps_are_counted():
    # code 1.5 * scale (1 + 2^-23) = 1.5 + 2^-23 + 2^-24: exact in float64, an f32 midpoint.  From
    # acc 0 the float64 sum is exact (one rounding: not ambiguous).  From acc -2^-80 it is inexact
    # and rounds back onto the midpoint: a true FMA rounds down, the double rounding ties up.
    q = torch.zeros(QBLOCK, dtype=torch.uint8)
    q[0] = 0x3C
    s = torch.tensor([1.0 + 2.0 ** -23])
    acc, amb = ref_dequant_reduce([q], [s])
    assert amb == 0 and float(acc[0]) == 1.5 + 2.0 ** -22      # ties to even
    acc0 = torch.zeros(QBLOCK)
    acc0[0] = -2.0 ** -80
    _, amb = ref_dequant_reduce([q], [s], acc0=acc0)
    assert amb == 1


def test_truncating_conversion_differs():
    x = _data(QBLOCK * 6, 2)
    q, s = ref_quant(x)
    codes = torch.arange(0, 0x7F, dtype=torch.int64).to(torch.uint8)       # the finite magnitudes
    mags = decode(codes)
    y = (x.view(-1, QBLOCK) * (1.0 / s)[:, None]).clamp(-448, 448).reshape(-1)
    idx = torch.bucketize(y.abs(), mags, right=True) - 1       # the largest magnitude <= |y|
    trunc = codes[idx] | (torch.signbit(y).to(torch.uint8) << 7)
    differ = int((trunc != q).sum())
    assert differ > x.numel() // 4                             # about half of all values round up
    assert (decode(trunc).abs() <= decode(q).abs()).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_ref_store_rounds_once(dtype):
    acc = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -0.0])
    out = ref_store(acc, dtype)
    assert out.dtype == dtype
    if dtype == torch.bfloat16:                                # 7 mantissa bits: ties at 2^-8
        assert out.float().tolist()[:2] == [1.0, 1.0 + 2.0 ** -6]
    if dtype == torch.float16:                                 # 10 mantissa bits: ties at 2^-11
        assert out.float().tolist()[2:4] == [1.0, 1.0 + 2.0 ** -9]
    if dtype == torch.float32:
        assert torch.equal(out, acc)
    assert torch.signbit(out[4])
