"""An independent reference of the block-scaled e4m3 codec (K6), in plain torch on the CPU.

It shares no code with csrc/kernels/fp8.hpp: the kernels are compared with it bit for bit
(tests/test_fp8_codec_gpu.py), and tests/test_fp8_ref_cpu.py keeps the reference itself honest.

The format: 256 elements per f32 scale, whole blocks (a partial last block is zero-padded).
  scale = amax / 448 in f32 (1.0 for a block whose amax is 0), amax ignoring NaN;
  code  = e4m3fn(clamp(x * (1 / scale), -448, 448)), round to nearest even; NaN stays NaN (0x7f).
  dequant-reduce: acc = fma(code_k, scale_k, acc) in f32, k in input order.
"""
import torch

QBLOCK = 256
FP8_MAX = 448.0


def nblocks(n: int) -> int:
    return (n + QBLOCK - 1) // QBLOCK


def ref_quant(x: torch.Tensor):
    """(q uint8[nblk * 256], scales f32[nblk]) of x (f32 / bf16 / f16, any n)."""
    xf = x.detach().cpu().reshape(-1).to(torch.float32)       # exact for bf16 / f16
    n = xf.numel()
    nblk = nblocks(n)
    pad = torch.zeros(nblk * QBLOCK, dtype=torch.float32)
    pad[:n] = xf
    b = pad.view(nblk, QBLOCK)
    a = b.abs()
    amax = torch.where(torch.isnan(a), torch.zeros_like(a), a).amax(dim=1)
    scale = torch.where(amax > 0, amax / torch.tensor(FP8_MAX, dtype=torch.float32),
                        torch.ones_like(amax))
    inv = torch.ones_like(scale) / scale                      # f32, correctly rounded
    y = (b * inv[:, None]).clamp(-FP8_MAX, FP8_MAX)           # clamp passes NaN through
    q = y.to(torch.float8_e4m3fn).view(torch.uint8).reshape(-1)
    return q, scale


def decode(q: torch.Tensor) -> torch.Tensor:
    """The exact f32 value of every e4m3fn code."""
    return q.detach().cpu().contiguous().view(torch.float8_e4m3fn).to(torch.float32)


def ref_dequant_reduce(qs, ss, acc0=None):
    """(acc f32[nblk * 256], ambiguous): acc = fma(code_k, scale_k, acc) for k in input order, from
    0 or from acc0 (f32, at most nblk * 256 elements, zero-padded).

    Every step is computed in float64 — the product of a 4-bit and a 24-bit significand is exact,
    so the step is ONE rounded float64 add — and rounded to f32.  That equals the f32 FMA unless
    the float64 sum was inexact AND landed exactly on an f32 midpoint; `ambiguous` counts those
    steps.  A test asserts it is 0 for its inputs (a condition on the inputs: change the seed, never
    the comparison)."""
    ntot = qs[0].numel()
    assert ntot % QBLOCK == 0, "whole blocks"
    acc = torch.zeros(ntot, dtype=torch.float32)
    if acc0 is not None:
        a0 = acc0.detach().cpu().reshape(-1).to(torch.float32)
        acc[:a0.numel()] = a0
    ambiguous = 0
    for q, s in zip(qs, ss):
        assert q.numel() == ntot and s.numel() == ntot // QBLOCK
        c = decode(q).to(torch.float64)
        sc = s.detach().cpu().to(torch.float32).to(torch.float64).repeat_interleave(QBLOCK)
        prod = c * sc                                          # exact
        a = acc.to(torch.float64)
        t = a + prod
        bb = t - a                                             # TwoSum: err = the add's rounding error
        err = (a - (t - bb)) + (prod - bb)
        mid = (t.view(torch.int64) & 0x1FFFFFFF) == 0x10000000
        ambiguous += int((torch.isfinite(t) & (err != 0) & mid).sum())
        acc = t.to(torch.float32)
    return acc, ambiguous


def ref_store(acc: torch.Tensor, dtype) -> torch.Tensor:
    """The f32 accumulators stored as f32 / bf16 / f16: one round to nearest even."""
    return acc.to(dtype)
