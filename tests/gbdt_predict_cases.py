"""Fixed forests of the GBDT prediction tests (K18), shared by the CPU and the GPU file.  The sizes come
from csrc/kernels/gbdt_walk_map.hpp: a chunk holds 512 nodes, a row tile 1024 rows, F = 45 is the smallest F
whose bins are read from global memory."""
import torch

from mp4x.parallel.gbdt import GbdtForest

CHUNK_NODES, ROW_TILE, GLOBAL_F = 512, 1024, 45
# +-0, denormals, and magnitudes so far apart that another order of addition gives other bits
VALUES = [0.0, -0.0, 5e-324, -2.5e-310, 1.0, 1e16, -1e16, 3.0, 1e-8, -1e300, 1e300, 0.1, -7.25, 2.0 ** -1060]
THRESHOLDS = [-1, 254, 255, 2 ** 31 - 1, -2 ** 31, -9]


def heap_tree(size, F, salt):
    """``size`` node rows of a complete binary tree (node i has the children 2i + 1 and 2i + 2 while both exist)."""
    rows = []
    for i in range(size):
        thr = THRESHOLDS[(i + salt) % len(THRESHOLDS)] if (i + salt) % 5 == 0 else (i * 53 + salt * 17) % 255
        rows.append([(i * 5 + salt) % F, thr, 2 * i + 1, 2 * i + 2] if 2 * i + 2 < size else [-1, -1, -1, -1])
    return rows


def _forest(trees, steps, off=None):
    rows = [r for t in trees for r in t]
    sizes = torch.tensor([0] + [len(t) for t in trees])
    value = torch.tensor([VALUES[(i * 7 + 3) % len(VALUES)] for i in range(len(rows))], dtype=torch.float64)
    off = torch.cumsum(sizes, 0).to(torch.int32) if off is None else torch.tensor(off, dtype=torch.int32)
    return GbdtForest(torch.tensor(rows, dtype=torch.int32).reshape(-1, 4), value, off, steps)


def forest(kind, F):
    if kind == "no_trees":
        return _forest([], 6)
    if kind == "one_leaf":
        return _forest([heap_tree(1, F, 0)], 0)
    if kind == "cross_a_chunk":                       # 5 trees of 127 nodes: four fit a chunk, the fifth crosses
        return _forest([heap_tree(127, F, t) for t in range(5)], 6)
    if kind == "big_then_small":                      # the global walk, then LDS chunks again, in order
        return _forest([heap_tree(CHUNK_NODES + 1, F, 1)] + [heap_tree(7, F, t) for t in range(3)], 9)
    if kind == "hostile_nodes":                       # a self-loop | a two-node cycle | children outside | feature >= F
        return _forest([[[0, 100, 0, 0]], [[0, -2 ** 31, 1, 1], [0, 2 ** 31 - 1, 0, 0], [-1, 0, -1, -1]],
                        [[0, 50, 1, 2], [0, 0, 5, 0], [0, 0, 0, -4]], [[F, 7, 1, 1], [0, 7, 0, 0]]], 9)
    if kind == "hostile_offsets":                     # negative, non-monotone, past N; six trees' nodes under them
        return _forest([heap_tree(7, F, t) for t in range(6)], 3, off=[99, -5, 7, 3, 2 ** 31 - 1, 12, -2 ** 31, 42])
    raise KeyError(kind)


FORESTS = ["no_trees", "one_leaf", "cross_a_chunk", "big_then_small", "hostile_nodes", "hostile_offsets"]
ROWS = [1, ROW_TILE - 1, ROW_TILE + 1, 2 * ROW_TILE + 17]
# (forest, n, F, init): every n at every LDS F for the two forests that cross chunks, a diagonal for the rest,
# F = 45 (bins from global memory) with about 300 rows for all; init None, given, or given and aliased by pred
CASES = [(k, n, F) for k in ("cross_a_chunk", "big_then_small") for n in ROWS for F in (1, 3, 37)] + \
    [(k, n, F) for k in ("no_trees", "one_leaf", "hostile_nodes", "hostile_offsets") for n, F in zip(ROWS, (3, 37, 1, 3))] + \
    [(k, 301, GLOBAL_F) for k in FORESTS]
CASES = [c + (("none", "given", "alias")[i % 3],) for i, c in enumerate(CASES)]


def rows_case(n, F):
    """``(bins, init)``: bins over all 256 values (0, 255 and missing-value bins past any B), one column of 0 and
    255 alone."""
    gen = torch.Generator().manual_seed(100 * n + F)
    bins = torch.randint(0, 256, (n, F), dtype=torch.uint8, generator=gen)
    bins[:, F // 2] = torch.where(torch.arange(n) % 2 == 0, 0, 255).to(torch.uint8)
    init = torch.tensor([VALUES[(r * 3 + 1) % len(VALUES)] for r in range(n)], dtype=torch.float64)
    return bins, init
