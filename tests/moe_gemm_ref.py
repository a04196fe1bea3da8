"""What the tests of the grouped expert GEMM share (tests/test_moe_gemm_cpu.py today, a kernel's tests
when there is one): the float64 definition from exactly converted inputs, its bound, and the case
generators.

    out[r]  = act(x[r] . W[g] + bias[g])          for the rows r group g owns, +0 where mask <= 0
    gW[g]   = sum_r x[r]^T . gy[r],  gb[g] = sum_r gy[r]

f32 / bf16 / f16 inputs convert to float64 exactly and every product of two of them is exact there.
A float32 sum of n products plus the bias, in any order, with or without FMA, puts a term through at
most n + 1 roundings of at most one f32 ulp each (2^-23 relative: nothing is assumed about the MFMA's
internal rounding but that), so the f32 value errs by at most

    bound = (n + 2) * 2^-23 * (sum |a * b| + |bias|),    n = the reduction length (Kd, N or the rows)

to first order with a term to spare.  ReLU and the mask do not grow an error.  The one rounding to
the output dtype then adds u * (|v| + bound), u = 2^-8 (bf16), 2^-11 (f16), 2^-24 (f32).  Neither is
tuned."""
import torch

from fp8_rsag_ref import same_bits  # noqa: F401  (re-exported for the tests)

ULP32 = 2.0 ** -23
U_OUT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}


# ---------------------------------------------------------------- segment tables
def ragged(lengths, tail=0):
    """(table, R, segments): group g owns ``lengths[g]`` rows, ``tail`` rows behind them are nobody's."""
    offsets = [0]
    for n in lengths:
        offsets.append(offsets[-1] + n)
    segs = [[(offsets[g], lengths[g])] for g in range(len(lengths))]
    return ("ragged", torch.tensor(offsets, dtype=torch.int64)), offsets[-1] + tail, segs


def padded(valid, S):
    """(table, R, segments) of ``valid`` [G][B] (values above S are clamped by the kernel) and S."""
    G, B = len(valid), len(valid[0])
    segs = [[((g * B + b) * S, max(0, min(valid[g][b], S))) for b in range(B)] for g in range(G)]
    return ("padded", torch.tensor(valid, dtype=torch.int64), S), G * B * S, segs


def owned(segs, R):
    """bool [R]: the rows somebody owns."""
    m = torch.zeros(R, dtype=torch.bool)
    for group in segs:
        for lo, n in group:
            m[lo:lo + n] = True
    return m


def table_to(table, device):
    return (table[0], table[1].to(device)) + tuple(table[2:])


def shaped(t, table):
    """[R, width] as the layout's tensor: [G, B*S, width] along a padded table."""
    if table[0] == "padded":
        return t.reshape(table[1].shape[0], table[1].shape[1] * table[2], t.shape[-1])
    return t


# ---------------------------------------------------------------- the definition
def forward(x, w, segs, bias=None, act=None, transpose_w=False, mask=None):
    """(out float64 [R, N], bound float64 [R, N]) from ``x`` [R, Kd] and ``w`` as the call gets it;
    both 0 in the rows nobody owns, whatever ``x`` and ``mask`` hold there."""
    x64, w64 = x.reshape(-1, x.shape[-1]).to(torch.float64), w.to(torch.float64)
    if transpose_w:
        w64 = w64.transpose(1, 2)
    Kd, N = w64.shape[1], w64.shape[2]
    out, bound = torch.zeros(x64.shape[0], N, dtype=torch.float64), torch.zeros(x64.shape[0], N, dtype=torch.float64)
    for g, group in enumerate(segs):
        for lo, n in group:
            if n == 0:
                continue
            v = x64[lo:lo + n] @ w64[g]
            mag = x64[lo:lo + n].abs() @ w64[g].abs()
            if bias is not None:
                v, mag = v + bias[g].to(torch.float64), mag + bias[g].to(torch.float64).abs()
            if act == "relu":
                v = torch.relu(v)
            bd = (Kd + 2) * ULP32 * mag
            if mask is not None:
                dead = mask.reshape(-1, N)[lo:lo + n].to(torch.float64) <= 0
                v, bd = torch.where(dead, torch.zeros_like(v), v), torch.where(dead, torch.zeros_like(bd), bd)
            out[lo:lo + n], bound[lo:lo + n] = v, bd
    return out, bound


def wgrad(x, gy, segs):
    """(gw [G, Kd, N], its bound, gb [G, N], its bound), float64."""
    x64, g64 = x.reshape(-1, x.shape[-1]).to(torch.float64), gy.reshape(-1, gy.shape[-1]).to(torch.float64)
    G, Kd, N = len(segs), x64.shape[1], g64.shape[1]
    gw, bw = torch.zeros(G, Kd, N, dtype=torch.float64), torch.zeros(G, Kd, N, dtype=torch.float64)
    gb, bb = torch.zeros(G, N, dtype=torch.float64), torch.zeros(G, N, dtype=torch.float64)
    for g, group in enumerate(segs):
        rows = sum(n for _, n in group)
        for lo, n in group:
            if n == 0:
                continue
            gw[g] += x64[lo:lo + n].t() @ g64[lo:lo + n]
            bw[g] += x64[lo:lo + n].abs().t() @ g64[lo:lo + n].abs()
            gb[g] += g64[lo:lo + n].sum(0)
            bb[g] += g64[lo:lo + n].abs().sum(0)
        bw[g] *= (rows + 2) * ULP32
        bb[g] *= (rows + 2) * ULP32
    return gw, bw, gb, bb


def inside(got, want64, bound, dtype):
    """(ok, the worst reached fraction of the allowance) of ``got`` in ``dtype`` against the
    definition: |got - want| <= bound + u * (|want| + bound).  An exact match passes a zero bound."""
    allow = bound + U_OUT[dtype] * (want64.abs() + bound)
    err = (got.detach().to(torch.float64).cpu().reshape(want64.shape) - want64).abs()
    if err.numel() == 0:
        return True, 0.0
    ratio = torch.where(err == 0, torch.zeros_like(err), err / allow.clamp(min=1e-300))
    return bool((err <= allow).all()), float(ratio.max())


# ---------------------------------------------------------------- data
def integers(shape, a, b, c, dtype):
    """Integers in [-4, 4]: element (i, j, k) of a [.., .., ..] tensor is ((a*i + b*j + c*k) mod 9) - 4
    over the last three (or fewer) dimensions: asymmetric in every pair of indices."""
    idx = torch.meshgrid(*[torch.arange(n) for n in shape], indexing="ij")
    coef = (a, b, c)[3 - len(shape):]
    v = sum(q * i for q, i in zip(coef, idx))
    return ((v % 9) - 4).to(dtype)


def values(shape, dtype, seed, scale=1.0):
    """Random signs times magnitudes uniform in ``scale * [0.5, 2)``: the whole significand is used and
    sums cancel, but no product is tiny.  The output-rounding term u * |v| above holds for normal
    numbers only; a float16 result below 2^-14 rounds with an absolute error of up to 2^-25 instead.
    With every |a * b| >= scale_a * scale_b / 4 and the scales used here (1, and Kd^-1/2 for weights
    that are summed over Kd >= 8 products) every sum |a * b| is at least 1/4, so the bound itself is at
    least 3 * 2^-23 / 4 > 2^-25 and covers that case as well."""
    g = torch.Generator().manual_seed(seed)
    sign = torch.randint(0, 2, shape, generator=g).to(torch.float32) * 2 - 1
    return (sign * (0.5 + 1.5 * torch.rand(*shape, generator=g)) * scale).to(dtype)


def poison(t, keep, fill):
    """``t`` [R, width] with ``fill`` in every row where ``keep`` [R] is False."""
    out = t.clone()
    out[~keep] = fill
    return out
