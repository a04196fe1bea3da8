"""Fixed cases of the GBDT binning tests (K19), shared by the CPU and the GPU file.  The sizes come from
csrc/kernels/gbdt_bin_map.hpp: a block serves 64 features and a row tile of 4096 rows; E = 63 | 64 changes the
number of search steps, E = 255 is the cap."""
import math

import torch

ROW_TILE, NAN, INF = 4096, math.nan, math.inf
TINY, DEN = 1e-45, 1e-40            # float32 denormals: the smallest one and a larger one

# name -> (edges of one feature, cnt, missing, the values x, their bins)
TABLE = {
    "x_equal_to_an_edge": ([1.0, 2.0, 3.0], 3, 255, [0.5, 1.0, 1.5, 2.0, 3.0, 4.0], [0, 1, 1, 2, 3, 3]),
    "minus_zero_edge": ([-0.0], 1, 255, [0.0, -0.0, -TINY], [1, 1, 0]),
    "plus_zero_edge": ([0.0], 1, 255, [-0.0, 0.0, -TINY], [1, 1, 0]),
    "denormals": ([-TINY, TINY, DEN], 3, 255, [-TINY, 0.0, TINY, 5e-41, DEN, 1e-38, -DEN], [1, 1, 2, 2, 3, 3, 0]),
    "infinities": ([-INF, 0.0, INF], 3, 255, [-INF, -1.0, INF, 3e38], [1, 1, 3, 2]),
    "nan_x": ([1.0], 1, 7, [NAN, -NAN, 2.0], [7, 7, 1]),
    "nan_edge": ([1.0, NAN, 3.0], 3, 255, [0.0, 5.0], [0, 1]),
    "unsorted_edges": ([5.0, 1.0, 3.0], 3, 255, [2.0, 0.0, 6.0], [2, 0, 3]),
    "cnt_negative": ([1.0, 2.0, 3.0], -4, 255, [5.0], [0]),
    "cnt_past_E": ([1.0, 2.0, 3.0], 2 ** 31 - 1, 255, [2.5, 5.0], [2, 3]),
    "cnt_1_of_3": ([1.0, 2.0, 3.0], 1, 255, [5.0], [1]),
    "no_edges": ([], 0, 255, [1.0, NAN], [0, 255]),
}


def table_case(name):
    """``(X [m, 1], edges [1, E], cnt [1], missing, want [m, 1])`` of a row of TABLE."""
    edges, cnt, missing, xs, want = TABLE[name]
    return (torch.tensor(xs, dtype=torch.float32)[:, None], torch.tensor(edges, dtype=torch.float32).reshape(1, len(edges)),
            torch.tensor([cnt], dtype=torch.int32), missing, torch.tensor(want, dtype=torch.uint8)[:, None])


SPECIALS = [NAN, INF, -INF, 0.0, -0.0, TINY, -TINY, DEN, 65504.0, 6e-8]
# (n, F, E, dtype): every n at F = 130 and every F at two tiles + 17 cross each row and feature boundary once, the
# E on both sides of a step count and the cap ride along; one case each of float16 and bfloat16
CASES = [(1, 130, 255, torch.float32), (ROW_TILE - 1, 3, 64, torch.float32), (ROW_TILE + 1, 65, 63, torch.float32),
         (2 * ROW_TILE + 17, 37, 255, torch.float32), (2 * ROW_TILE + 17, 130, 2, torch.float32),
         (ROW_TILE + 1, 64, 1, torch.float32), (300, 1, 0, torch.float32), (300, 1, 255, torch.float32),
         (ROW_TILE + 1, 3, 2, torch.float32), (300, 64, 64, torch.float32), (2 * ROW_TILE + 17, 65, 0, torch.float32),
         (ROW_TILE + 1, 37, 63, torch.float16), (ROW_TILE - 1, 130, 255, torch.bfloat16)]


def bin_case(n, F, E, dtype):
    """``(X, edges, cnt)`` on the CPU.  Features are ascending edges with some of SPECIALS among them and ``cnt``
    anywhere in ``[0, E]``, but feature 0 has unsorted edges, feature 1 NaN edges, and every fifth a hostile
    ``cnt``; X draws from the edges themselves, values between them and SPECIALS."""
    gen = torch.Generator().manual_seed(1000 * n + 10 * F + E)
    special = torch.tensor(SPECIALS, dtype=torch.float32)
    edges = torch.randn(F, E, generator=gen) * 3
    if E:
        plant = torch.rand(F, E, generator=gen) < 0.1
        edges = torch.where(plant, special[3:][torch.randint(0, len(SPECIALS) - 3, (F, E), generator=gen)], edges)
        edges = edges.to(dtype).to(torch.float32).sort(dim=1).values
        edges[0] = edges[0][torch.randperm(E, generator=gen)]
        if F > 1:
            edges[1, ::3] = NAN
    cnt = torch.randint(0, E + 1, (F,), generator=gen).to(torch.int32)
    cnt[::2] = E
    cnt[4::5] = torch.tensor([-5, E + 9, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32).repeat(F)[:len(cnt[4::5])]
    X = torch.randn(n, F, generator=gen) * 3
    if E:
        pick = torch.randint(0, E, (n, F), generator=gen)
        X = torch.where(torch.rand(n, F, generator=gen) < 0.3, edges.t().gather(0, pick), X)
    X = torch.where(torch.rand(n, F, generator=gen) < 0.05, special[torch.randint(0, len(SPECIALS), (n, F), generator=gen)], X)
    return X.to(dtype).contiguous(), edges.contiguous(), cnt


def edges_case(n, dtype=torch.float32):
    """X ``[n, 7]``: normal values | a constant | all NaN | four tied values | +-0 and denormals | +-inf among
    values | NaN sprinkled over values."""
    gen = torch.Generator().manual_seed(n)
    r = torch.randn(n, 7, generator=gen)
    pick = torch.randint(0, 4, (n,), generator=gen)
    cols = [r[:, 0], torch.full((n,), 2.5), torch.full((n,), NAN), pick.to(torch.float32),
            torch.tensor([0.0, -0.0, TINY, -DEN])[pick], torch.where(r[:, 5] > 1, INF, torch.where(r[:, 5] < -1, -INF, r[:, 5])),
            torch.where(r[:, 0] > 0.5, NAN, r[:, 6])]
    return torch.stack(cols, dim=1).to(dtype)


def brute_edges(X, B):
    """The definition of ``gbdt_edges`` by a plain sort of every whole column, as ``(edges, cnt)`` lists."""
    edges, cnt = [], []
    for col in X.to(torch.float32).t():
        vals = sorted(0.0 if v == 0 else v for v in col.tolist() if v == v)
        cand = sorted({vals[q * len(vals) // B] for q in range(1, B)}) if vals else []
        edges.append(cand + [INF] * (B - 1 - len(cand)))
        cnt.append(len(cand))
    return edges, cnt
