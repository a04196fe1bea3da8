"""What the tests of the fused combine backward (K11, tests/test_moe_combine_bwd_*.py) share: the
float64 definition of the gate weights' gradient, its bound, and the slot generators.

    g_weights[t, k] = sum_h g[t, h] * rows[slots[t*K + k], h]      (0 where the slot is < 0)

The f32 / bf16 / f16 inputs convert to float64 exactly, and every product of two of them is exact in
float64, so the float64 sum is the exact value to 2^-53 relative of sum |g * y|.  A float32 dot
product of n terms, in any order and with or without contraction to FMA, rounds every product at
most once and every partial sum at most once per addition: a term passes through at most n roundings,
so the result errs by at most n * u / (1 - n * u) * sum |g * y| with u = 2^-24 (Higham's gamma_n),
which is below (n + 2) * u * sum |g * y| while n^2 * u + 2 * n * u <= 2, that is for every n <= 4096
(the widths tested here; a longer row is covered to first order, and K11's own order, W * ceil(V / G)
terms per lane and a tree of log2 G steps, puts a term through far fewer than n roundings).  Hence
gamma = (width + 2) * 2^-24 (DESIGN "K11"); it is not tuned.
"""
import torch

import moe_padded_ref
import moe_ref

U = 2.0 ** -24


def gamma(width):
    return (width + 2) * U


def definition(g, rows, slots, K):
    """(g_weights float64 [T, K], bound float64 [T, K]) of ``g`` [T, H], ``rows`` [R, H] and ``slots``
    int64 [T*K]; both 0 where the slot is negative (rows may hold anything there, NaN included)."""
    T = g.shape[0]
    H = g[0].numel() if T else rows[0].numel()
    sl = slots.view(T, K)
    live = sl >= 0
    if rows.shape[0] == 0:                                    # nothing was kept: every slot is -1
        rows = torch.zeros((1, H), dtype=rows.dtype)
    y = rows.reshape(rows.shape[0], H).to(torch.float64)[sl.clamp(min=0)]                 # [T, K, H]
    y = torch.where(live.unsqueeze(-1), y, torch.zeros_like(y))
    prod = g.reshape(T, 1, -1).to(torch.float64) * y
    return prod.sum(-1), gamma(H) * prod.abs().sum(-1)


def torch_f32(g, rows, slots, K):
    """The float32 CPU evaluation of the same inputs: the expression of ``_Combine.backward``."""
    T = g.shape[0]
    sl = slots.view(T, K)
    y = rows.reshape(rows.shape[0], g[0].numel())[sl.clamp(min=0)].to(torch.float32)
    g_w = (g.reshape(T, 1, -1).to(torch.float32) * y).sum(-1)
    return torch.where(sl >= 0, g_w, torch.zeros_like(g_w))


def inside(got, want64, bound):
    """(ok, worst ratio) of |got - want64| <= bound elementwise (an exact match passes a zero bound)."""
    err = (got.detach().to(torch.float64).cpu().reshape(want64.shape) - want64).abs()
    if err.numel() == 0:
        return True, 0.0
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp(min=1e-300))
    return bool((err <= bound).all()), float(ratio.max())


def zero_bits_where_clipped(got, slots):
    """Every clipped assignment's gradient is +0.0 by its bits."""
    dead = (slots < 0).reshape(-1)
    return bool((got.detach().cpu().reshape(-1).view(torch.int32)[dead] == 0).all())


# ---------------------------------------------------------------- slots
def ragged_ids(T, K, E, seed):
    """Expert ids [T, K] in [0, E): their slots (moe_ref.ref_route) are a bijection onto [0, T*K)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, E, (T, K), generator=g)


def clipped_ids(T, K, E, seed, share=0.25):
    """ragged_ids with about ``share`` of the assignments at -1 and the middle token clipped whole."""
    g = torch.Generator().manual_seed(seed + 1)
    ids = ragged_ids(T, K, E, seed)
    ids[torch.rand(T, K, generator=g) < share] = -1
    ids[T // 2] = -1
    return ids


def ragged_slots(ids, E):
    """(slots int64 [T*K], the number of rows they name)."""
    _, slots, order = moe_ref.ref_route(ids, E)
    return slots, int(order.numel())


def padded_slots(ids, E, S):
    """slots ``e*S + pe`` of the padded layout (-1 past the share S); E*S rows, which may exceed T*K."""
    return moe_padded_ref.cut_ids(ids, E, S)[1]


def values(n, width, dtype, seed, scale=1.0):
    """Normally distributed rows that use the whole significand of ``dtype``."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, width, generator=g) * scale).to(dtype)


def cancelling(T, width, dtype, seed):
    """(g [T, width], rows [2T, width], slots [T*2]) with K = 2: the elements of g come in equal pairs,
    slot (t, 0) names the row +g, -g, +g, ... whose products with g cancel exactly, slot (t, 1) names g."""
    g = values(T, width // 2, dtype, seed).repeat_interleave(2, dim=1)
    sign = torch.tensor([1.0, -1.0]).repeat(width // 2)
    rows = torch.cat([(g.to(torch.float32) * sign).to(dtype), g])
    return g, rows, torch.arange(2 * T).view(2, T).t().reshape(-1).contiguous()


def weights(T, K, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(T, K, generator=g) * 2 - 0.5
