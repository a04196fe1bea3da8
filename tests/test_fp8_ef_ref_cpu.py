"""tests/fp8_ef_ref.py kept honest without a GPU: with a zero residual it is fp8_ref.ref_quant, the
sum of what it sends telescopes to the sum of its inputs, and on the drift case it recovers the
elements the memoryless quantiser drops on every step."""
import pytest

torch = pytest.importorskip("torch")

from fp8_ef_ref import DRIFT_N, DRIFT_T, drift_input, ref_dequant, ref_quant_ef  # noqa: E402
from fp8_ref import QBLOCK, nblocks, ref_quant  # noqa: E402

FLOATS = [torch.float32, torch.bfloat16, torch.float16]
_ids = lambda v: str(v).replace("torch.", "")  # noqa: E731


def _data(n, seed, dtype=torch.float32):
    """randn * logspace(-3, 3) with a negative amax and a few -0.0 planted."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g) * torch.logspace(-3, 3, n)
    first = min(n, QBLOCK)
    x[first // 2] = -2.0 * float(x[:first].abs().max())
    x[1] = -0.0
    if n >= 4 * QBLOCK:
        x[3 * QBLOCK + torch.tensor([0, 17, 255])] = -0.0
    return x.to(dtype)


@pytest.mark.parametrize("dtype", FLOATS, ids=_ids)
@pytest.mark.parametrize("n", [4, 260, 256 * 9 + 100])
def test_zero_residual_is_ref_quant_except_negative_zero(dtype, n):
    x = _data(n, 3 + n, dtype)
    q0, s0 = ref_quant(x)
    q, s, r, amb = ref_quant_ef(x, torch.zeros(n))
    assert amb == 0
    assert torch.equal(s.view(torch.int32), s0.view(torch.int32))
    negz = torch.zeros(nblocks(n) * QBLOCK, dtype=torch.bool)
    negz[:n] = x.float().view(torch.int32) == -2 ** 31            # the bits of -0.0
    assert int(negz.sum()) >= 1
    assert torch.equal(q[~negz], q0[~negz])
    assert (q0[negz] == 0x80).all() and (q[negz] == 0).all()      # -0 + +0 = +0
    assert not q[n:].any()                                        # the pad: zero codes
    assert r.dtype == torch.float32 and r.numel() == n and torch.isfinite(r).all()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_sent_sum_telescopes_to_the_input_sum(seed):
    """sum_t dequant(q_t) = sum_t x_t + r_0 - r_T per element, to within the rounding of the T f32
    adds x_t + r_{t-1}: T * 2^-24 * max_t |x_t + r_{t-1}|."""
    T, n = 8, 1000
    g = torch.Generator().manual_seed(100 + seed)
    r0 = torch.randn(n, generator=g) * 1e-2
    r = r0.clone()
    sent = torch.zeros(n, dtype=torch.float64)
    total = torch.zeros(n, dtype=torch.float64)
    xe_max = torch.zeros(n, dtype=torch.float64)
    for t in range(T):
        x = _data(n, 1000 * seed + t, [torch.float32, torch.bfloat16, torch.float16][seed]).float() * 1e-2
        xe_max = torch.maximum(xe_max, (x + r).abs().double())
        q, s, r, amb = ref_quant_ef(x, r)
        assert amb == 0
        sent += ref_dequant(q, s, n)
        total += x.double()
    gap = (sent - (total + r0.double() - r.double())).abs()
    bound = T * 2.0 ** -24 * xe_max
    assert (gap <= bound).all(), (float((gap - bound).max()), int((gap > bound).sum()))


def test_nonfinite_inputs_reset_the_residual():
    n = 3 * QBLOCK
    x = _data(n, 9)
    r0 = torch.randn(n, generator=torch.Generator().manual_seed(10)) * 1e-3
    qc, sc, rc, _ = ref_quant_ef(x, r0)
    x[5] = float("nan")                                           # block 0: its own element only
    x[2 * QBLOCK + 7] = float("-inf")                             # block 2: the whole block
    q, s, r, _ = ref_quant_ef(x, r0)
    assert r[5] == 0 and (r[2 * QBLOCK:] == 0).all()
    keep = torch.ones(n, dtype=torch.bool)
    keep[5] = False
    keep[2 * QBLOCK:] = False
    assert torch.equal(r[keep].view(torch.int32), rc[keep].view(torch.int32))
    assert torch.equal(q[:2 * QBLOCK][keep[:2 * QBLOCK]], qc[:2 * QBLOCK][keep[:2 * QBLOCK]])
    assert torch.isfinite(r).all()


def test_drift_case():
    """A constant gradient for 64 steps: element 1 (1e-6 next to a 1.0) is below half the block's
    smallest code step, so the memoryless quantiser sends 0 for it on every step; with error
    feedback its sent sum is within one code step of 64e-6."""
    g = drift_input()
    assert g.numel() == DRIFT_N and float(g[1]) == pytest.approx(1e-6)
    plain = torch.zeros(DRIFT_N, dtype=torch.float64)
    sent = torch.zeros(DRIFT_N, dtype=torch.float64)
    r = torch.zeros(DRIFT_N)
    for _ in range(DRIFT_T):
        q0, s0 = ref_quant(g)
        plain += ref_dequant(q0, s0, DRIFT_N)
        q, s, r, amb = ref_quant_ef(g, r)
        assert amb == 0
        sent += ref_dequant(q, s, DRIFT_N)
    assert float(plain[1]) == 0.0
    step = float(s[0]) * 2.0 ** -9                                # block 0's smallest code step
    assert float(g[1]) < step / 2
    assert abs(float(sent[1]) - 64e-6) <= step, (float(sent[1]), step)
    # the whole vector: with feedback the accumulated error is the final residual (telescoping),
    # without it every element repeats its rounding error 64 times
    true = g.double() * DRIFT_T
    err_ef, err_plain = (sent - true).abs().max(), (plain - true).abs().max()
    print(f"drift: accumulated error {float(err_plain):.3e} without feedback, {float(err_ef):.3e} with, "
          f"final residual {float(r.abs().max()):.3e}")
    assert float(err_ef) <= float(r.abs().max()) + DRIFT_T * 2.0 ** -24 * 3.0
