"""The fp8 quantiser with error feedback (k_quant_ef: csrc/kernels/codec.hip, device_ops.quant_fp8_ef)
against the CPU reference of tests/fp8_ef_ref.py, bit for bit: codes, scales and the new residual
as integers.  Nothing here has a tolerance."""
import pytest

torch = pytest.importorskip("torch")

from fp8_ef_ref import DRIFT_N, DRIFT_T, drift_input, ref_quant_ef  # noqa: E402
from fp8_ref import QBLOCK, nblocks  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
FLOATS = [torch.float32, torch.bfloat16, torch.float16]
SIZES = [4, 252, 256, 260, 1024, 1028, 256 * 9 + 100]
_IVIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
_ids = lambda v: str(v).replace("torch.", "")  # noqa: E731
CANARY_F, CANARY_Q = 7.25, 0xA5
PAD = 64            # canary elements on either side of every buffer (256 bytes of f32: 16-byte aligned)


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


def _resid(n, seed, x):
    """A residual of the size one step leaves: up to a sixteenth of the element, either sign."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, generator=g) - 0.5) * 0.125 * x.float().abs().clamp(min=1e-4)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(_IVIEW[t.dtype]) if t.dtype in _IVIEW else t


def _eq_i(got, ref, what=""):
    got, ref = _bits(got), _bits(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = got != ref
    assert not bad.any(), (what, int(bad.sum()), bad.nonzero().view(-1)[:8].tolist())


def _same_codes(got, ref, what=""):
    """Equal codes; a NaN code (0x7f / 0xff) only has to be a NaN code at the same place."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    rn = (ref & 0x7F) == 0x7F
    bad = torch.where(rn, (got & 0x7F) != 0x7F, got != ref)
    assert not bad.any(), (what, int(bad.sum()), bad.nonzero().view(-1)[:8].tolist())


class _Bufs:
    """resid, q and scales for n elements, each between two canary runs."""

    def __init__(self, n, resid):
        self.n, self.nblk = n, nblocks(n)
        self.rbig = torch.full((n + 2 * PAD,), CANARY_F, dtype=torch.float32, device=DEV)
        self.qbig = torch.full((self.nblk * QBLOCK + 2 * PAD,), CANARY_Q, dtype=torch.uint8, device=DEV)
        self.sbig = torch.full((self.nblk + 2 * PAD,), CANARY_F, dtype=torch.float32, device=DEV)
        self.r = self.rbig[PAD:PAD + n]
        self.q = self.qbig[PAD:PAD + self.nblk * QBLOCK]
        self.s = self.sbig[PAD:PAD + self.nblk]
        self.r.copy_(resid)
        assert self.r.data_ptr() % 16 == 0

    def canaries_intact(self):
        for big, inner, c in ((self.rbig, self.n, CANARY_F), (self.qbig, self.nblk * QBLOCK, CANARY_Q),
                              (self.sbig, self.nblk, CANARY_F)):
            assert (big[:PAD] == c).all() and (big[PAD + inner:] == c).all()


def _step(K, x, bufs, what=""):
    """One device step on ``bufs`` against the reference: codes, scales, residual, pad, input, canaries."""
    n = x.numel()
    r_in = bufs.r.cpu()
    rq, rs, rr, amb = ref_quant_ef(x, r_in)
    assert amb == 0, what          # a condition on the inputs: change a seed, never the comparison
    xd = x.to(DEV)
    q, s = K.quant_fp8_ef(xd, bufs.r, bufs.q, bufs.s)
    torch.cuda.synchronize()
    assert q is bufs.q and s is bufs.s
    _eq_i(bufs.s, rs, what + " scales")
    _same_codes(bufs.q, rq, what + " codes")
    assert not bufs.q[n:].any(), what + " pad codes"
    _eq_i(bufs.r, rr, what + " residual")
    _eq_i(xd, x, what + " input")
    bufs.canaries_intact()


@pytest.mark.parametrize("dtype", FLOATS, ids=_ids)
@pytest.mark.parametrize("n", SIZES)
def test_quant_ef_bit_exact(dtype, n):
    """Zero residual, a random residual, and two chained steps on the residual the first left."""
    K, _ = _K()
    x = _data(n, 11 + n, dtype)
    _step(K, x, _Bufs(n, torch.zeros(n)), "zero residual")
    bufs = _Bufs(n, _resid(n, 5 + n, x))
    _step(K, x, bufs, "random residual")
    _step(K, _data(n, 12 + n, dtype, plant=False), bufs, "chained step 1")
    _step(K, _data(n, 13 + n, dtype), bufs, "chained step 2")


def test_quant_ef_allocates_whole_blocks_like_quant_fp8():
    K, _ = _K()
    n = 260
    x = _data(n, 3)
    r = torch.zeros(n, device=DEV)
    q, s = K.quant_fp8_ef(x.to(DEV), r)
    rq, rs, rr, _ = ref_quant_ef(x, torch.zeros(n))
    assert q.numel() == n and s.numel() == 2 and q.untyped_storage().nbytes() >= 2 * QBLOCK
    _eq_i(q, rq[:n])
    _eq_i(s, rs)
    _eq_i(r, rr)


def test_nonfinite_inputs_reset_their_residual_only():
    """A NaN resets its own residual element, an infinity its whole block (the block's scale is
    infinite); the blocks next to them are those of a clean run."""
    K, _ = _K()
    n = 5 * QBLOCK
    x = _data(n, 21, plant=False)
    r0 = _resid(n, 22, x)
    clean = _Bufs(n, r0)
    _step(K, x, clean, "clean")
    y = x.clone()
    y[QBLOCK + 9] = float("nan")                  # block 1
    y[3 * QBLOCK + 100] = float("inf")            # block 3
    bufs = _Bufs(n, r0)
    _step(K, y, bufs, "planted")
    got, ref = bufs.r.cpu(), clean.r.cpu()
    assert got[QBLOCK + 9] == 0 and (got[3 * QBLOCK:4 * QBLOCK] == 0).all()
    assert torch.isfinite(got).all()
    same = torch.ones(n, dtype=torch.bool)
    same[QBLOCK + 9] = False
    same[3 * QBLOCK:4 * QBLOCK] = False
    _eq_i(got[same], ref[same], "residual next to the planted values")
    for b in (0, 2, 4):
        sl = slice(b * QBLOCK, (b + 1) * QBLOCK)
        _eq_i(bufs.q[sl], clean.q[sl], f"codes of block {b}")
        _eq_i(bufs.s[b:b + 1], clean.s[b:b + 1], f"scale of block {b}")
    # the step after: the reset block starts from zero, nothing is poisoned
    _step(K, x, bufs, "step after")
    assert torch.isfinite(bufs.r).all()


def test_quant_ef_grid_stride_bit_exact():
    """The capped grid-stride form with more blocks than one sweep of the grid, a ragged tail."""
    K, lib = _K()
    n = 256 * (32768 + 5) + 8
    x = _data(n, 5)
    bufs = _Bufs(n, _resid(n, 6, x))
    try:
        lib.mp4x_set_codec_grid(0)
        _step(K, x, bufs, "grid-stride")
        torch.cuda.synchronize()
    finally:
        lib.mp4x_set_codec_grid(1)


def test_drift_case_on_the_device():
    """The drift case of tests/test_fp8_ef_ref_cpu.py through the kernel, step by step."""
    K, _ = _K()
    g = drift_input()
    gd = g.to(DEV)
    r_ref = torch.zeros(DRIFT_N)
    r = torch.zeros(DRIFT_N, device=DEV)
    q = torch.empty(nblocks(DRIFT_N) * QBLOCK, dtype=torch.uint8, device=DEV)
    s = torch.empty(nblocks(DRIFT_N), device=DEV)
    got = []
    for _ in range(DRIFT_T):
        K.quant_fp8_ef(gd, r, q, s)
        got.append((q.clone(), s.clone(), r.clone()))
    torch.cuda.synchronize()
    for t, (qd, sd, rd) in enumerate(got):
        rq, rs, r_ref, amb = ref_quant_ef(g, r_ref)
        assert amb == 0
        _eq_i(qd, rq, f"step {t} codes")
        _eq_i(sd, rs, f"step {t} scales")
        _eq_i(rd, r_ref, f"step {t} residual")


def test_refusals_write_nothing():
    K, lib = _K()
    n = 512
    x = _data(n, 2).to(DEV)
    bufs = _Bufs(n + 4, torch.full((n + 4,), 0.5))
    before = (bufs.rbig.clone(), bufs.qbig.clone(), bufs.sbig.clone())
    bad = {
        "dtype": bufs.r[:n].to(torch.float16),
        "short": bufs.r[:n - 4],
        "off by 4 bytes": bufs.r[1:n + 1],
        "not contiguous": torch.zeros(2 * n, device=DEV)[::2],
        "host": torch.zeros(n),
    }
    assert bad["off by 4 bytes"].data_ptr() % 16 == 4
    for what, res in bad.items():
        with pytest.raises(ValueError):
            K.quant_fp8_ef(x, res, bufs.q, bufs.s)
    with pytest.raises(ValueError):
        K.quant_fp8_ef(x[:510], bufs.r[:510], bufs.q, bufs.s)                  # n % 4 != 0
    # the C entry point refuses the same by itself (a caller that is not the wrapper)
    from mp4x.operators import DType
    f32 = int(DType.F32)
    qp, sp, rp, xp = bufs.q.data_ptr(), bufs.s.data_ptr(), bufs.r.data_ptr(), x.data_ptr()
    assert lib.mp4x_quant_fp8_ef(f32, xp, 510, rp, qp, sp, None) == 1001
    assert lib.mp4x_quant_fp8_ef(f32, xp, n, rp + 4, qp, sp, None) == 1001
    assert lib.mp4x_quant_fp8_ef(f32, xp, n, None, qp, sp, None) == 1001
    assert lib.mp4x_quant_fp8_ef(f32, xp, n, rp, None, sp, None) == 1001
    assert lib.mp4x_quant_fp8_ef(f32, xp, n, rp, qp, None, None) == 1001
    assert lib.mp4x_quant_fp8_ef(f32, None, n, rp, qp, sp, None) == 1001
    assert lib.mp4x_quant_fp8_ef(int(DType.F64), xp, n, rp, qp, sp, None) == 1002
    torch.cuda.synchronize()
    for now, then in zip((bufs.rbig, bufs.qbig, bufs.sbig), before):
        assert torch.equal(now, then)
