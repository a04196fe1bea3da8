"""Fixed cases of the GBDT tests (K16), shared by the CPU and the GPU files."""
import numpy as np
import torch

QMAX = 2 ** 31 - 1
BIG = 2 ** 62
HOSTILE = {"past_m": [5, 9, 4, 1000, 12], "negative": [0, -3, 7, 7, -1], "huge": [BIG, -BIG, 3, BIG, -1]}

# (g, sg) and (h, sh): +-0, denormals, products on k + 1/2 for even and odd k, the value just below 2**30,
# values past the declared range (clamp), +-inf, NaN; sh < 0 shifts right
QUANT_G = ([0.0, -0.0, 1e-45, -1e-45, 2.5 / 1024, 3.5 / 1024, -2.5 / 1024, -3.5 / 1024, (2 ** 20 + 0.5) / 1024,
            float(np.nextafter(np.float32(2 ** 20), np.float32(0))), 2.0 ** 21, 3e6, -3e6, float("inf"), float("-inf"),
            float("nan"), 0.3], 10)
QUANT_H = ([4.0, -4.0, 12.0, 20.0, -12.0, -20.0, 1.0, 1e30, -1e30, 2.0 ** 34, 2.0 ** 34 - 2048, float("nan"),
            float("inf"), 0.0, 7.0, 8.0, 1e-45], -3)


def hist_case(n, F, B, k, seed=0, one_node=False, one_bin=False, bad_rows=False, high_bins=False, seg=None):
    """bins, gh, rows, seg on the CPU.  Rows are spread over the k nodes and one inactive bucket (k = 64:
    over three nodes only); ``seg``: a hostile table over a permutation of all rows instead."""
    gen = torch.Generator().manual_seed(1000 * seed + n + F + B + k)
    bins = torch.randint(0, min(256, B + 3) if high_bins else B, (n, F), dtype=torch.uint8, generator=gen)
    if one_bin:
        bins[:] = B - 1
    gh = torch.randint(-QMAX, QMAX + 1, (n, 2), dtype=torch.int32, generator=gen)
    if seg is not None:
        return bins, gh, torch.randperm(n, generator=gen).to(torch.int32), torch.tensor(seg, dtype=torch.int64)
    live = torch.tensor([3, 40, 63, k]) if k == 64 else torch.arange(k + 1)
    node = torch.zeros(n, dtype=torch.int64) if one_node else live[torch.randint(0, len(live), (n,), generator=gen)]
    rows = torch.sort(node, stable=True).indices[:int((node < k).sum())].to(torch.int32)
    offs = torch.zeros(k + 1, dtype=torch.int64)
    offs[1:] = torch.cumsum(torch.bincount(node, minlength=k + 1)[:k], 0)
    if bad_rows:
        rows[::7] = -1
        rows[3::11] = n
        rows[5::13] = rows[1].item()
    return bins, gh, rows, offs


def guarded(shape, dtype, device, guard=4):
    """(buffer, view): the view is the output, ``guard`` sentinel elements stand on either side."""
    numel = int(np.prod(shape))
    buf = torch.full((numel + 2 * guard,), 77, dtype=dtype, device=device)
    return buf, buf[guard:guard + numel].view(shape)


def guards_intact(buf, guard=4):
    return bool((buf[:guard] == 77).all()) and bool((buf[-guard:] == 77).all())


def _hist(cols):
    """int64 [1, F, B, 2] from per-feature lists of (g, h) pairs."""
    return torch.tensor([cols], dtype=torch.int64)


_COL = [(-100, 10), (30, 5), (-7, 3), (90, 12)]
# name -> (hist, sg, sh, lam, feature, threshold)
SPLIT = {
    "identical_columns": (_hist([_COL, _COL]), 0, 0, 1.0, 0, 0),
    "plateau": (_hist([[(-100, 10), (0, 0), (0, 0), (100, 10)]]), 0, 0, 1.0, 0, 0),
    "second_feature_wins": (_hist([[(1, 10), (1, 10), (1, 10), (1, 10)], _COL]), 3, 2, 1.0, 1, 0),
    "two_bins": (_hist([[(-64, 4), (64, 4)]]), 4, 1, 0.5, 0, 0),
    "empty_node": (_hist([[(0, 0)] * 4] * 2), 0, 0, 1.0, -1, -1),
    "empty_node_lam0": (_hist([[(0, 0)] * 4] * 2), 0, 0, 0.0, -1, -1),
    "zero_hessian_lam0": (_hist([[(5, 0), (-5, 0), (9, 0)]]), 0, 0, 0.0, -1, -1),
}


def random_hist(k, F, B, seed):
    gen = torch.Generator().manual_seed(seed)
    g = torch.randint(-2 ** 40, 2 ** 40, (k, F, B), generator=gen)
    h = torch.randint(0, 50, (k, F, B), generator=gen) << 29
    return torch.stack([g, h], dim=3)


def model_data():
    """The data of tests/test_models.py's GBDT test, bins as bytes."""
    from mp4x.models.gbdt import quantize
    rng = np.random.default_rng(5)
    X = rng.normal(size=(900, 5))
    y = np.sin(X[:, 0]) + X[:, 1] ** 2 + 0.1 * rng.normal(size=900)
    return quantize(X, 16)[0], y


def tree_tuple(t):
    return (t.feature, t.threshold, t.left, t.right, t.value)
