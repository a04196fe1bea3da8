"""What the tests of the gated (SwiGLU) expert activation share (tests/test_moe_glu_cpu.py today, a
kernel's tests when there is one): the float64 definition from exactly converted inputs, its three
bounds, the segment tables, the data and the edge fixture.

    h[r, j]         = silu(g) * u                      g = pre[r, j], u = pre[r, N + j]
    g_pre[r, j]     = g_h * u * silu'(g)               silu'(g) = s(g) * (1 + g * s(-g)), s = 1 / (1 + exp(-.))
    g_pre[r, N + j] = g_h * silu(g)

for the rows somebody owns; 0 in the others, whatever the inputs hold there.

The bounds on the float32 value before the rounding to the dtype, u24 = 2^-24, for |g| <= 32.  They
follow the router gate's B_sigma = 16 u24 for 1 / (1 + exp) (an exp within 2 ulp of an argument of at
most 32, one addition, one division): a product or quotient adds u24 each.

    forward   g / (1 + exp(-g)) is B_sigma + the division's own, times u:            18 u24 |h|
    g_up      the same quotient times g_h, with a term to spare:                     20 u24 |g_up|
    g_gate    two sigmoids (32 u24), g * sm, 1 + ., s * ., g_h * u, the last product;
              silu' has a zero near g = -1.2785, so the bound is absolute in
              A = |g_h| |u| s(g) (1 + |g| s(-g)) >= |g_gate|:                        40 u24 A

None is tuned.  The rounding to the dtype is added by ``moe_gemm_ref.inside``: u (|v| + bound).  That
term holds for normal results only.  silu(-32) is -4e-13, so at scale 16 a float16 result can lie below
2^-14, where float16 rounds with an absolute error of up to half its subnormal spacing, 2^-25 (see
``moe_gemm_ref.values``); :func:`inside` here adds that half spacing of the dtype (2^-25, 2^-134, 2^-150)
to the bound of the elements whose float64 value lies below the dtype's smallest normal number, and of
no other.  It is a property of the number format."""
import torch

import moe_gemm_ref
from moe_gemm_ref import U_OUT, owned, padded, poison, ragged, shaped, table_to, values  # noqa: F401
from moe_gemm_ref import same_bits  # noqa: F401

U24 = 2.0 ** -24
BOUNDS = {"h": 18, "g_up": 20, "g_gate": 40}              # in units of u24
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
TINY = {dt: torch.finfo(dt).tiny for dt in DTYPES}        # the smallest normal number
HALF_SUBNORMAL = {torch.float16: 2.0 ** -25, torch.bfloat16: 2.0 ** -134, torch.float32: 2.0 ** -150}


def inside(got, want64, bound, dtype):
    """``moe_gemm_ref.inside`` with the dtype's half subnormal spacing added to the bound where the
    float64 value is below the dtype's smallest normal number (a value the bound could carry across
    that line is counted too)."""
    below = (want64.abs() - bound) < TINY[dtype]
    return moe_gemm_ref.inside(got, want64, bound + below.to(bound.dtype) * HALF_SUBNORMAL[dtype], dtype)


def _sig(x):
    return 1.0 / (1.0 + torch.exp(-x))


def forward64(pre, own):
    """(h float64 [R, N], its bound) from ``pre`` [R, 2N] in any of the dtypes; 0 where ``own`` [R] is False."""
    p = pre.reshape(-1, pre.shape[-1]).to(torch.float64)
    N = p.shape[1] // 2
    g, u = p[:, :N], p[:, N:]
    h = (g * _sig(g)) * u
    keep = own.view(-1, 1).expand_as(h)
    h = torch.where(keep, h, torch.zeros_like(h))
    return h, BOUNDS["h"] * U24 * h.abs()


def backward64(pre, g_h, own):
    """(g_pre float64 [R, 2N], its bound) from ``pre`` [R, 2N] and ``g_h`` [R, N]."""
    p = pre.reshape(-1, pre.shape[-1]).to(torch.float64)
    d = g_h.reshape(-1, g_h.shape[-1]).to(torch.float64)
    N = p.shape[1] // 2
    g, u = p[:, :N], p[:, N:]
    s, sm = _sig(g), _sig(-g)
    gg = d * u * s * (1.0 + g * sm)
    A = d.abs() * u.abs() * s * (1.0 + g.abs() * sm)
    gu = d * (g * s)
    out = torch.cat([gg, gu], dim=1)
    bound = torch.cat([BOUNDS["g_gate"] * U24 * A, BOUNDS["g_up"] * U24 * gu.abs()], dim=1)
    keep = own.view(-1, 1).expand_as(out)
    zero = torch.zeros_like(out)
    return torch.where(keep, out, zero), torch.where(keep, bound, zero)


# ---------------------------------------------------------------- tables
def tables():
    """name -> (table, R, segments): the tables of the kernel tests."""
    g = torch.Generator().manual_seed(70)
    rnd = torch.randint(-2, 76, (2, 4), generator=g).tolist()
    rnd[0][0], rnd[1][3] = -2, 75                                    # both ends occur
    out = {"padded S=5": padded([[0, 5], [7, -1], [3, 1]], 5),
           "padded 1x1x1 valid": padded([[1]], 1),
           "padded 1x1x1 empty": padded([[0]], 1),
           "padded 2x4 S=70": padded(rnd, 70),
           "ragged": ragged([0, 3, 65, 0, 1]),
           "ragged +4": ragged([0, 3, 65, 0, 1], tail=4)}
    # non-monotone and negative: c = [0, 9, 9, 20, 20, 20] over R = 23; too large: c = [0, 2, 6, 6] over R = 6
    out["ragged non-monotone"] = (("ragged", torch.tensor([5, 9, 4, 20, 12, -7], dtype=torch.int64)), 23,
                                  [[(0, 9)], [(9, 0)], [(9, 11)], [(20, 0)], [(20, 0)]])
    out["ragged too large"] = (("ragged", torch.tensor([0, 2, 2 ** 62, 3], dtype=torch.int64)), 6,
                               [[(0, 2)], [(2, 4)], [(6, 0)]])
    out["no row"] = ragged([0, 0])
    return out


def case(table, R, segs, N, dtype, scale, seed):
    """(pre [R, 2N] along the table, g_h, own [R]): magnitudes ``scale * [0.5, 2)``, every row nobody
    owns NaN in both."""
    own = owned(segs, R)
    pre = poison(values((R, 2 * N), dtype, seed, scale), own, float("nan"))
    g_h = poison(values((R, N), dtype, seed + 1, scale), own, float("nan"))
    return shaped(pre, table), shaped(g_h, table), own


# ---------------------------------------------------------------- the float32 formula, as stated
def formula32(pre, g_h=None):
    """The stated float32 formula evaluated by torch on the CPU, before the rounding: ``h`` [R, N], or
    ``g_pre`` [R, 2N] with ``g_h``."""
    p = pre.reshape(-1, pre.shape[-1]).to(torch.float32).cpu()
    N = p.shape[1] // 2
    g, u = p[:, :N], p[:, N:]
    den = 1.0 + torch.exp(-g)
    if g_h is None:
        return (g / den) * u
    d = g_h.reshape(-1, N).to(torch.float32).cpu()
    s, sm = 1.0 / den, 1.0 / (1.0 + torch.exp(g))
    return torch.cat([(d * u) * (s * (1.0 + g * sm)), d * (g / den)], dim=1)


# ---------------------------------------------------------------- the edge fixture
EDGE_G = (0.0, -0.0, float("inf"), float("-inf"), float("nan"), 88.8, -88.8, -104.0)
EDGE_U = (0.0, -0.0, 1.0, -1.0, float("inf"), float("-inf"), float("nan"))
EDGE_N = 64                                       # 56 pairs and 8 ordinary ones: whole 16-byte vectors


def edge_case(dtype):
    """(pre [2, 128], g_h [2, 64], the ragged table that owns both rows): every pair (g, u) of the two
    lists, with g_h = 1.5 in row 0 and -0.75 in row 1."""
    gs = [g for g in EDGE_G for _ in EDGE_U] + [1.0] * (EDGE_N - len(EDGE_G) * len(EDGE_U))
    us = [u for _ in EDGE_G for u in EDGE_U] + [1.0] * (EDGE_N - len(EDGE_G) * len(EDGE_U))
    row = torch.tensor(gs + us, dtype=torch.float32)
    pre = torch.stack([row, row]).to(dtype)
    g_h = torch.stack([torch.full((EDGE_N,), 1.5), torch.full((EDGE_N,), -0.75)]).to(dtype)
    return pre, g_h, ("ragged", torch.tensor([0, 2], dtype=torch.int64))


def classes(t):
    """0 finite, 1 NaN, 2 +inf, 3 -inf."""
    t = t.to(torch.float32)
    c = torch.zeros(t.shape, dtype=torch.int64)
    c[torch.isnan(t)] = 1
    c[t == float("inf")] = 2
    c[t == float("-inf")] = 3
    return c


def edge_check(got, pre, g_h=None):
    """None, or what is wrong with ``got`` (``h``, or ``g_pre`` with ``g_h``) on the edge fixture.

    The class of every element is that of the stated float32 formula evaluated by torch on the CPU and
    rounded to the dtype.  A finite value lies inside its bound plus the dtype's smallest normal number
    around that evaluation.  The reference for the finite values is the float32 formula and not the
    float64 one because the fixture leaves the bounds' domain |g| <= 32 on purpose: at g = -88.8 the
    float32 expf(88.8) is +inf, the formula gives -0 and float64 gives -2.4e-37, thirty times the
    smallest normal float32.  Where g = +-0 (inside the domain) the float64 definition is held too."""
    dtype = pre.dtype
    want32 = formula32(pre, g_h)
    want = want32.to(dtype)
    got = got.detach().cpu().reshape(want.shape)
    if not torch.equal(classes(got), classes(want)):
        bad = (classes(got) != classes(want)).nonzero()[0].tolist()
        return f"class differs at {bad}: {float(got[tuple(bad)])} for {float(want[tuple(bad)])}"
    own = torch.ones(want.shape[0], dtype=torch.bool)
    w64, bound = forward64(pre, own) if g_h is None else backward64(pre, g_h, own)
    fin = classes(want) == 0
    bound = torch.where(torch.isfinite(bound), bound, torch.zeros_like(bound))
    # around the float32 evaluation: the bound scales with the value, so take it at the larger of the two
    ref = want32.to(torch.float64)
    N = pre.shape[-1] // 2
    if g_h is None:
        factor = torch.full_like(ref, BOUNDS["h"])
    else:                                            # each half of g_pre has its own factor
        factor = torch.cat([torch.full((ref.shape[0], N), float(BOUNDS["g_gate"]), dtype=ref.dtype),
                            torch.full((ref.shape[0], N), float(BOUNDS["g_up"]), dtype=ref.dtype)], dim=1)
    mag = factor * U24 * ref.abs()
    allow = torch.maximum(bound, mag) * (1 + U_OUT[dtype]) + U_OUT[dtype] * ref.abs() + TINY[dtype]
    err = (got.to(torch.float64) - ref).abs()
    if bool((err[fin] > allow[fin]).any()):
        return f"finite values off by up to {float((err[fin] / allow[fin]).max()):.3f} of the allowance"
    zero_g = (pre.reshape(-1, 2 * N)[:, :N].to(torch.float32) == 0)
    zero_g = zero_g if g_h is None else torch.cat([zero_g, zero_g], dim=1)
    sel = zero_g & fin & torch.isfinite(w64)
    allow64 = bound + U_OUT[dtype] * (w64.abs() + bound) + TINY[dtype]
    if bool(((got.to(torch.float64) - w64).abs()[sel] > allow64[sel]).any()):
        return "a value at g = +-0 is outside the float64 bound"
    return None
