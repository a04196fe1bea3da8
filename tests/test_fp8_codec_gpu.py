"""The block-scaled e4m3 codec (K6: csrc/kernels/fp8.hpp, codec.hip) against the independent CPU
reference of tests/fp8_ref.py, bit for bit: codes and scales as integers, outputs as their
storage.  Nothing here has a tolerance.  The fused fp8 IPC allreduce and the RCCL fp8 schedule are
tested against K6, so K6 is pinned here against something that is not K6."""
import pytest

torch = pytest.importorskip("torch")

from fp8_ref import QBLOCK, nblocks, ref_dequant_reduce, ref_quant, ref_store  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
FLOATS = [torch.float32, torch.bfloat16, torch.float16]
_IVIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
_ids = lambda v: str(v).replace("torch.", "")  # noqa: E731


def _K():
    from mp4x.ops import device_ops, native
    return device_ops, native.hip()


def _data(n, seed, dtype=torch.float32, plant=True):
    """randn * logspace(-3, 3) with the planted blocks: block 0 has a negative amax and a -0.0,
    block 1 is all zero, block 2 one repeated value, block 3 holds several -0.0."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g) * torch.logspace(-3, 3, n)
    if plant:
        first = min(n, QBLOCK)
        x[first // 2] = -2.0 * float(x[:first].abs().max())
        if n >= 8:
            x[1] = -0.0
        if n >= 2 * QBLOCK:
            x[QBLOCK:2 * QBLOCK] = 0.0
        if n >= 3 * QBLOCK:
            x[2 * QBLOCK:3 * QBLOCK] = 0.37
        if n >= 4 * QBLOCK:
            x[3 * QBLOCK + torch.tensor([0, 17, 255])] = -0.0
    return x.to(dtype)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(_IVIEW[t.dtype]) if t.dtype in _IVIEW else t


def _same(got, ref):
    """Equal storage, except that a NaN only has to be a NaN (payloads differ between an x86 and
    a GPU NaN, and after a bf16 / f16 store)."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.dtype == ref.dtype and got.shape == ref.shape
    gn, rn = torch.isnan(got), torch.isnan(ref)
    bad = (gn != rn) | (~rn & (_bits(got) != _bits(ref)))
    assert not bad.any(), (int(bad.sum()), bad.nonzero().view(-1)[:8].tolist())


def _same_codes(got, ref):
    """Equal codes; a NaN code (0x7f / 0xff) only has to be a NaN code at the same place."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    rn = (ref & 0x7F) == 0x7F
    bad = torch.where(rn, (got & 0x7F) != 0x7F, got != ref)
    assert not bad.any(), (int(bad.sum()), bad.nonzero().view(-1)[:8].tolist())


def _eq_i(got, ref):
    got, ref = _bits(got), _bits(ref)
    bad = got != ref
    assert got.shape == ref.shape and not bad.any(), (int(bad.sum()), bad.nonzero().view(-1)[:8].tolist())


# ---------------------------------------------------------------- 1. quant
def _check_quant(K, x):
    n = x.numel()
    nblk = nblocks(n)
    rq, rs = ref_quant(x)
    xd = x.to(DEV)
    q, s = K.quant_fp8(xd)
    assert q.numel() == n and s.numel() == nblk
    _eq_i(s, rs)
    _eq_i(q, rq[:n])
    # a caller's whole-block buffer: codes, and the pad of the last block written as zeros
    buf = torch.full((nblk * QBLOCK,), 0xA5, dtype=torch.uint8, device=DEV)
    s2 = torch.empty(nblk, device=DEV)
    q2, _ = K.quant_fp8(xd, buf, s2)
    assert q2 is buf
    _eq_i(s2, rs)
    _eq_i(buf, rq)
    assert not rq[n:].any()


@pytest.mark.parametrize("dtype", FLOATS, ids=_ids)
@pytest.mark.parametrize("n", [4, 252, 256, 260, 1024, 1028, 256 * 9 + 100])
def test_quant_bit_exact(dtype, n):
    """One lane, one lane short of a block, a block, the 4-block unroll boundary, ragged sizes."""
    K, _ = _K()
    _check_quant(K, _data(n, 11 + n, dtype))


def test_quant_grid_stride_bit_exact():
    """The capped grid-stride form of k_quant with more blocks than one sweep of the grid."""
    K, lib = _K()
    n = 256 * (32768 + 5) + 8
    x = _data(n, 5)
    try:
        lib.mp4x_set_codec_grid(0)
        _check_quant(K, x)
        torch.cuda.synchronize()
    finally:
        lib.mp4x_set_codec_grid(1)


# ---------------------------------------------------------------- 2. dequant
_SCALES = [1.0, 2.0 ** -10 * 1.2345, 3.7e3 / 448.0, 1e-20, 1.0 / 3.0, 6.5e4]


@pytest.mark.parametrize("dtype", FLOATS, ids=_ids)
@pytest.mark.parametrize("ragged", [0, 100, 252], ids=lambda r: f"tail{r}")
def test_dequant_every_code(dtype, ragged):
    """Every code 0..255 under a few scales (f16 overflows to Inf under the last), to every output
    dtype; aligned and with a partial last block.  Elements past n stay untouched."""
    K, _ = _K()
    nblk = len(_SCALES) + 1
    q = torch.arange(256, dtype=torch.int64).to(torch.uint8).repeat(nblk)
    s = torch.tensor(_SCALES + [0.75], dtype=torch.float32)
    n = nblk * QBLOCK if not ragged else (nblk - 1) * QBLOCK + ragged
    acc, amb = ref_dequant_reduce([q], [s])
    assert amb == 0
    out = torch.full((n + 8,), 7.0, dtype=dtype, device=DEV)
    K.dequant_fp8(q.to(DEV), s.to(DEV), n, out[:n])
    _same(out[:n], ref_store(acc, dtype)[:n])
    assert (out[n:] == 7.0).all()


# ---------------------------------------------------------------- 3. dequant-reduce
_N3 = 256 * 5 + 100        # 6 blocks: DU = 4 runs one full group and one clamped partial group
_INPUTS = {}


def _inputs(nin, n=_N3, seed=40):
    """nin quantised inputs (by the reference, so the test does not lean on k_quant), on the CPU
    and on the device; computed once per (nin, n) and never modified."""
    key = (nin, n, seed)
    if key not in _INPUTS:
        cq, cs = zip(*[ref_quant(_data(n, seed + k, plant=(k % 3 == 0))) for k in range(nin)])
        _INPUTS[key] = (list(cq), list(cs), [t.to(DEV) for t in cq], [t.to(DEV) for t in cs])
    return _INPUTS[key]


def _check_dr(K, nin, dtype, n=_N3):
    cq, cs, dq, ds = _inputs(nin, n)
    nblk = nblocks(n)
    acc, amb = ref_dequant_reduce(cq, cs)
    assert amb == 0
    rq, rs = ref_quant(acc)                       # of the f32 accumulators, not of the rounded out
    # a fresh out, with the fused re-quantisation
    out = torch.full((n + 8,), 7.0, dtype=dtype, device=DEV)
    qo = torch.full((nblk * QBLOCK,), 0xA5, dtype=torch.uint8, device=DEV)
    so = torch.empty(nblk, device=DEV)
    K.dequant_reduce_fp8(out[:n], dq, ds, n, q_out=qo, s_out=so)
    _same(out[:n], ref_store(acc, dtype)[:n])
    assert (out[n:] == 7.0).all()
    _eq_i(so, rs)
    _eq_i(qo, rq)
    # accumulate onto a non-zero out: the chain starts from out's value
    out0 = _data(n, 99).to(dtype)
    acc2, amb2 = ref_dequant_reduce(cq, cs, acc0=out0.float())
    assert amb2 == 0
    rq2, rs2 = ref_quant(acc2)
    out2 = out0.to(DEV)
    qo.fill_(0xA5)
    K.dequant_reduce_fp8(out2, dq, ds, n, accumulate=True, q_out=qo, s_out=so)
    _same(out2, ref_store(acc2, dtype)[:n])
    _eq_i(so, rs2)
    _eq_i(qo, rq2)
    # accumulate off ignores what out held
    out3 = out0.to(DEV)
    K.dequant_reduce_fp8(out3, dq, ds, n)
    _same(out3, ref_store(acc, dtype)[:n])
    # no out at all: only the re-quantised sum
    qo.fill_(0xA5)
    so.fill_(-1.0)
    K.dequant_reduce_fp8(None, dq, ds, n, q_out=qo, s_out=so, out_dtype=dtype)
    _eq_i(so, rs)
    _eq_i(qo, rq)


@pytest.mark.parametrize("dtype", FLOATS, ids=_ids)
@pytest.mark.parametrize("nin", [1, 2, 3, 4, 5, 6, 7, 8])
def test_dequant_reduce_bit_exact(nin, dtype):
    """The explicit FMA chain in input order at every fan-in of one launch (default unroll)."""
    K, _ = _K()
    _check_dr(K, nin, dtype)


@pytest.mark.parametrize("dtype", FLOATS, ids=_ids)
@pytest.mark.parametrize("nin", [1, 3, 8])
@pytest.mark.parametrize("du", [1, 2, 4])
def test_dequant_reduce_unrolls_bit_exact(du, nin, dtype):
    """Every unroll (quant blocks per wave iteration) at every fan-in class: each block keeps its
    own scale, and the clamped partial group of the last blocks writes nothing twice."""
    K, lib = _K()
    try:
        lib.mp4x_set_dq_unroll(du)
        _check_dr(K, nin, dtype)
        torch.cuda.synchronize()
    finally:
        lib.mp4x_set_dq_unroll(0)


def test_dequant_reduce_grid_stride_bit_exact():
    """More blocks than 8192 waves x DU: the wave loop of k_dequant_reduce iterates."""
    K, _ = _K()
    n = 256 * 16390
    cq, cs = zip(*[ref_quant(_data(n, 70 + k)) for k in range(2)])
    acc, amb = ref_dequant_reduce(cq, cs)
    assert amb == 0
    rq, rs = ref_quant(acc)
    out = torch.empty(n, device=DEV)
    qo = torch.empty(n, dtype=torch.uint8, device=DEV)
    so = torch.empty(n // QBLOCK, device=DEV)
    K.dequant_reduce_fp8(out, [t.to(DEV) for t in cq], [t.to(DEV) for t in cs], n, q_out=qo, s_out=so)
    _same(out, acc)
    _eq_i(so, rs)
    _eq_i(qo, rq)


# ---------------------------------------------------------------- 4. fan-in above one launch
def test_dequant_reduce_fan_in_11_is_one_chain():
    """11 inputs are two launches (8 + 3).  With f32 partial sums — an f32 out, or no out at all —
    the result is the single 11-step chain of the reference, exactly."""
    K, _ = _K()
    n = _N3
    nblk = nblocks(n)
    cq, cs, dq, ds = _inputs(11)
    acc, amb = ref_dequant_reduce(cq, cs)
    assert amb == 0
    rq, rs = ref_quant(acc)
    qo = torch.full((nblk * QBLOCK,), 0xA5, dtype=torch.uint8, device=DEV)
    so = torch.full((nblk,), -1.0, device=DEV)
    assert K.dequant_reduce_fp8(None, dq, ds, n, q_out=qo, s_out=so, out_dtype=torch.float32) is None
    _eq_i(so, rs)
    _eq_i(qo, rq)
    out = torch.empty(n, device=DEV)
    qo.fill_(0xA5)
    so.fill_(-1.0)
    K.dequant_reduce_fp8(out, dq, ds, n, q_out=qo, s_out=so)
    _same(out, acc[:n])
    _eq_i(so, rs)
    _eq_i(qo, rq)
    # the sum of the last launch alone (what an ignored accumulate leaves) is something else
    last, _ = ref_dequant_reduce(cq[8:], cs[8:])
    assert not torch.equal(ref_quant(last)[0], rq)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=_ids)
def test_dequant_reduce_fan_in_11_into_a_16_bit_out(dtype):
    """A bf16 / f16 out carries the partial sum between the launches itself, so the reference
    rounds once after the first 8 inputs and continues the chain from the rounded value: that
    intermediate rounding is part of the wrapper's contract (its docstring says so)."""
    K, _ = _K()
    n = _N3
    cq, cs, dq, ds = _inputs(11)
    head, amb = ref_dequant_reduce(cq[:8], cs[:8])
    acc, amb2 = ref_dequant_reduce(cq[8:], cs[8:], acc0=ref_store(head, dtype).float())
    assert amb == 0 and amb2 == 0
    out = torch.empty(n, dtype=dtype, device=DEV)
    K.dequant_reduce_fp8(out, dq, ds, n)
    _same(out, ref_store(acc, dtype)[:n])


# ---------------------------------------------------------------- 5. the buffer contract
def test_quant_writes_whole_blocks_and_nothing_else():
    """Whole blocks: q holds nblk * 256 bytes, the pad is written as zeros, the bytes on either
    side of it are not touched; a buffer of only n bytes is refused."""
    K, _ = _K()
    n = 256 * 3 + 4
    nblk = nblocks(n)
    x = _data(n, 21)
    rq, rs = ref_quant(x)
    big = torch.full((64 + nblk * QBLOCK + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    sbig = torch.full((nblk + 2,), -1.0, device=DEV)
    K.quant_fp8(x.to(DEV), big[64:64 + nblk * QBLOCK], sbig[1:1 + nblk])
    torch.cuda.synchronize()
    assert (big[:64] == 0xA5).all() and (big[64 + nblk * QBLOCK:] == 0xA5).all()
    assert float(sbig[0]) == -1.0 and float(sbig[-1]) == -1.0
    _eq_i(big[64:64 + nblk * QBLOCK], rq)
    _eq_i(sbig[1:1 + nblk], rs)
    with pytest.raises(ValueError):
        K.quant_fp8(x.to(DEV), big[64:64 + n], sbig[1:1 + nblk])
    with pytest.raises(ValueError):
        K.quant_fp8(x.to(DEV), torch.empty(n, dtype=torch.uint8, device=DEV))
    torch.cuda.synchronize()
    assert (big[64 + n:] == 0xA5).sum() == 64                   # the refused call wrote nothing
    # the codes quant_fp8 allocates itself are whole blocks with a zero pad, returned as [:n]
    q, s = K.quant_fp8(x.to(DEV))
    assert q.numel() == n
    base = q._base
    assert base is not None and base.numel() == nblk * QBLOCK and q.data_ptr() == base.data_ptr()
    _eq_i(base, rq)


def test_dequant_reduce_requant_refuses_short_buffers():
    K, _ = _K()
    n = 256 * 3 + 4
    nblk = nblocks(n)
    cq, cs = ref_quant(_data(n, 22))
    dq, ds = cq.to(DEV), cs.to(DEV)
    qo = torch.empty(nblk * QBLOCK, dtype=torch.uint8, device=DEV)
    so = torch.empty(nblk, device=DEV)
    out = torch.empty(n, device=DEV)
    with pytest.raises(ValueError):                            # q_out of n bytes
        K.dequant_reduce_fp8(out, [dq], [ds], n, q_out=qo[:n], s_out=so)
    with pytest.raises(ValueError):                            # s_out one short
        K.dequant_reduce_fp8(out, [dq], [ds], n, q_out=qo, s_out=so[:nblk - 1])
    short = dq[:n].clone()                                     # an allocation of n bytes: no pad behind it
    with pytest.raises(ValueError):
        K.dequant_reduce_fp8(out, [short], [ds], n, q_out=qo, s_out=so)
    # the n-byte view of whole blocks that quant_fp8 returns is accepted, and garbage-free
    x = _data(n, 23)
    q, s = K.quant_fp8(x.to(DEV))
    rq, rs = ref_quant(x)
    acc, amb = ref_dequant_reduce([rq], [rs])
    assert amb == 0
    K.dequant_reduce_fp8(out, [q], [s], n, q_out=qo, s_out=so)
    _same(out, acc[:n])
    _eq_i(qo, ref_quant(acc)[0])
    _eq_i(so, ref_quant(acc)[1])


# ---------------------------------------------------------------- 6. non-finite inputs
@pytest.mark.parametrize("dtype", FLOATS, ids=_ids)
def test_nan_and_inf_stay_non_finite(dtype):
    """A NaN element decodes to NaN and the rest of its block is what the reference gives with it
    ignored in the amax; a block with an infinity stores an infinite scale and decodes non-finite
    throughout; an all-NaN block has scale 1 and decodes to NaN; the finite blocks next to them
    are untouched."""
    K, _ = _K()
    n = 6 * QBLOCK
    clean = _data(n, 31, dtype, plant=False)
    x = clean.clone()
    x[QBLOCK + 10] = float("nan")
    x[QBLOCK + 255] = float("nan")
    x[3 * QBLOCK + 3] = float("inf")
    x[3 * QBLOCK + 77] = float("-inf")
    x[3 * QBLOCK + 78] = float("nan")
    x[5 * QBLOCK:] = float("nan")
    rq, rs = ref_quant(x)
    cq, cs = ref_quant(clean)
    q, s = K.quant_fp8(x.to(DEV))
    _eq_i(s, rs)
    assert float(s[3]) == float("inf") and float(s[5]) == 1.0
    _same_codes(q, rq)
    for b in (0, 2, 4):                                        # the neighbours: as if nothing was there
        _eq_i(q[b * QBLOCK:(b + 1) * QBLOCK], cq[b * QBLOCK:(b + 1) * QBLOCK])
        assert float(s[b]) == float(cs[b])
    y = torch.empty(n, device=DEV)
    K.dequant_fp8(q, s, n, y)
    acc, amb = ref_dequant_reduce([rq], [rs])
    assert amb == 0
    _same(y, acc)
    y = y.cpu()
    nan1 = torch.zeros(QBLOCK, dtype=torch.bool)
    nan1[[10, 255]] = True
    assert torch.equal(torch.isnan(y[QBLOCK:2 * QBLOCK]), nan1)
    assert torch.isfinite(y[QBLOCK:2 * QBLOCK][~nan1]).all()
    assert not torch.isfinite(y[3 * QBLOCK:4 * QBLOCK]).any()
    assert torch.isnan(y[5 * QBLOCK:]).all()
    for b in (0, 2, 4):
        assert torch.isfinite(y[b * QBLOCK:(b + 1) * QBLOCK]).all()


def test_nan_survives_the_fused_requantisation():
    """A NaN accumulator of the dequant-reduce re-quantises to a NaN code, and the block's scale
    comes from its finite accumulators."""
    K, _ = _K()
    n = 2 * QBLOCK
    xs = [_data(n, 33 + k, plant=False) for k in range(3)]
    xs[1][7] = float("nan")
    cq, cs = zip(*[ref_quant(x) for x in xs])
    acc, amb = ref_dequant_reduce(cq, cs)
    assert amb == 0 and int(torch.isnan(acc).sum()) == 1
    rq, rs = ref_quant(acc)
    out = torch.empty(n, device=DEV)
    qo = torch.empty(n, dtype=torch.uint8, device=DEV)
    so = torch.empty(2, device=DEV)
    K.dequant_reduce_fp8(out, [t.to(DEV) for t in cq], [t.to(DEV) for t in cs], n, q_out=qo, s_out=so)
    _same(out, acc)
    _eq_i(so, rs)
    _same_codes(qo, rq)
