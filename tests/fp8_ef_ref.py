"""The CPU reference of the fp8 quantiser with error feedback (k_quant_ef), built on tests/fp8_ref.py
(imported, never edited), and the drift case the tests share.

Per element, with r the f32 residual the rank keeps between calls:
  xe        = f32(x) + r                               one f32 add
  (q, s)    = ref_quant(xe)
  new_r     = xe + (-(decode(q) * s))                  ONE rounding (the kernel's FMA), 0 where not finite

The subtraction is written as the addition of the negated product so that the zero signs are the
FMA's.  The product of a 4-bit and a 24-bit significand is exact in float64, so the step is one
rounded float64 add, rounded again to f32; that equals the f32 FMA unless the float64 add was
inexact AND landed on an f32 midpoint.  ``ambiguous`` counts those elements, as
``fp8_ref.ref_dequant_reduce`` does; a test asserts it is 0 for its inputs (a condition on the
inputs: change a seed, never the comparison).
"""
import torch

from fp8_ref import QBLOCK, decode, nblocks, ref_quant


def ref_quant_ef(x: torch.Tensor, resid: torch.Tensor):
    """(q uint8[nblk * 256], scales f32[nblk], new_resid f32[n], ambiguous) of x (f32 / bf16 / f16)
    and the f32 residual of the same length."""
    xf = x.detach().cpu().reshape(-1).to(torch.float32)          # exact for bf16 / f16
    r = resid.detach().cpu().reshape(-1)
    assert r.dtype == torch.float32 and r.numel() == xf.numel()
    n = xf.numel()
    xe = xf + r                                                  # one f32 add
    q, s = ref_quant(xe)
    a = xe.to(torch.float64)
    sc = s.to(torch.float64).repeat_interleave(QBLOCK)[:n]
    prod = -(decode(q)[:n].to(torch.float64) * sc)               # exact
    t = a + prod
    bb = t - a                                                   # TwoSum: err = the add's rounding error
    err = (a - (t - bb)) + (prod - bb)
    mid = (t.view(torch.int64) & 0x1FFFFFFF) == 0x10000000
    ambiguous = int((torch.isfinite(t) & (err != 0) & mid).sum())
    new = t.to(torch.float32)
    new = torch.where(torch.isfinite(new), new, torch.zeros_like(new))
    return q, s, new, ambiguous


def ref_dequant(q: torch.Tensor, s: torch.Tensor, n: int) -> torch.Tensor:
    """decode(q) * s in float64 (exact), the first n elements."""
    return decode(q)[:n].to(torch.float64) * s.to(torch.float64).repeat_interleave(QBLOCK)[:n]


# ---------------------------------------------------------------- the drift case
DRIFT_N, DRIFT_T = 512, 64


def drift_input() -> torch.Tensor:
    """A constant gradient whose small elements the memoryless quantiser drops on every step: 1e-6
    everywhere, one large element per block, and a ramp so that some codes round up, some down."""
    g = torch.full((DRIFT_N,), 1e-6, dtype=torch.float32)
    g[2:256] = torch.linspace(1e-7, 5e-3, 254)
    g[258:] = torch.linspace(1e-7, 5e-3, 254)
    g[0] = 1.0
    g[256] = -3.0
    return g


assert nblocks(DRIFT_N) == 2
