"""Fixed cases of the tests of the GBDT walk over float features (K20), shared by the CPU and the GPU file.  The
forests are gbdt_predict_cases'; the tile rule is csrc/kernels/gbdt_fwalk_map.hpp's: 256 threads own 4, 2 or 1 rows
each, as many as keep the tile's keys (rows of F | 1 dwords) inside 45056 bytes, so F = 43 is the largest F staged
in LDS and F = 44 the smallest read from global memory (1024 rows a block there)."""
import math

import torch

import gbdt_predict_cases as pcases
from mp4x.parallel import gbdt

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
LDS_F, GLOBAL_F = 43, 44
SPECIALS = [math.nan, -math.nan, math.inf, -math.inf, 0.0, -0.0, 1e-45, -1e-45, 1e-40, 6e-8, 65504.0, 3e38]


def tile(F):
    return next((256 * U for U in (4, 2, 1) if (F | 1) * 4 * 256 * U <= 45056), 1024)


def edges_case(F, dtype, hand):
    """``(edges, cnt)``.  ``hand``: E = 6 with, in turn, ``cnt = 0`` | ``cnt = E`` and repeated edges | ``cnt = 3`` before
    a descending, NaN rest that no bin reads.  Else :func:`gbdt_edges` of 600 rows with B = 256, so the forests'
    thresholds below 255 name real edges, but for feature 1 (five distinct values) and feature 2 (all NaN)."""
    if hand:
        rows = [([5.0, 4.0, math.nan, 1.0, 0.0, -1.0], 0), ([-2.5, -0.0, 0.0, 0.0, 1e-40, math.inf], 6),
                ([-1.0, 0.5, 0.5, math.nan, 0.25, -3.0], 3)]
        pick = [rows[f % 3] for f in range(F)]
        return torch.tensor([e for e, _ in pick], dtype=torch.float32), torch.tensor([c for _, c in pick], dtype=torch.int32)
    gen = torch.Generator().manual_seed(F)
    train = torch.randn(600, F, generator=gen) * 3
    if F > 1:
        train[:, 1] = torch.randint(0, 5, (600,), generator=gen).float() - 2
    if F > 2:
        train[:, 2] = math.nan
    return gbdt.gbdt_edges(None, train.to(dtype), 256)


def rows_case(n, F, dtype, edges):
    """``(X, init)``: a third of X is an edge or one of its float32 neighbours, a tenth one of SPECIALS, the rest
    normal values; feature F // 2 alternates NaN and an ordinary value."""
    gen = torch.Generator().manual_seed(100 * n + F)
    X = torch.randn(n, F, generator=gen) * 3
    if edges.shape[1]:
        e = edges.nan_to_num(nan=1.0, posinf=math.inf, neginf=-math.inf).t().gather(0, torch.randint(0, edges.shape[1], (n, F), generator=gen))
        toward = torch.tensor([-math.inf, 0.0, math.inf])[torch.randint(0, 3, (n, F), generator=gen)]
        X = torch.where(torch.rand(n, F, generator=gen) < 0.33, torch.nextafter(e, torch.where(toward == 0, e, toward)), X)
    special = torch.tensor(SPECIALS)[torch.randint(0, len(SPECIALS), (n, F), generator=gen)]
    X = torch.where(torch.rand(n, F, generator=gen) < 0.1, special, X)
    X[::2, F // 2] = math.nan
    init = torch.tensor([pcases.VALUES[(r * 3 + 1) % len(pcases.VALUES)] for r in range(n)], dtype=torch.float64)
    return X.to(dtype).contiguous(), init


def case(kind, n, F, dtype, hand=False):
    """``(X, init, forest, edges, cnt)`` on the CPU, ``forest`` with bin thresholds."""
    edges, cnt = edges_case(F, dtype, hand)
    return rows_case(n, F, dtype, edges) + (pcases.forest(kind, F), edges, cnt)


# (forest, n, F): every n (around one and two tiles of that F) at every F for the two forests that cross chunks, F =
# 13 being one of two rows a lane; a diagonal for the rest.  The dtype and init (None, given, aliased by pred)
# cycle at different rates.
CASES = [(k, n, F) for k in ("cross_a_chunk", "big_then_small") for F in (1, 3, 13, LDS_F, GLOBAL_F)
         for n in (1, tile(F) - 1, tile(F) + 1, 2 * tile(F) + 17)] + \
    [(k, (1, tile(F) - 1, tile(F) + 1, 2 * tile(F) + 17)[i], F)
     for i, (k, F) in enumerate(zip(("no_trees", "one_leaf", "hostile_nodes", "hostile_offsets"), (3, LDS_F, 1, GLOBAL_F)))]
CASES = [c + (DTYPES[i % 3], ("none", "given", "alias")[(i // 2) % 3]) for i, c in enumerate(CASES)]
