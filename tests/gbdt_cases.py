"""Fixed cases of the GBDT tests (K16), shared by the CPU and the GPU files."""
import json
import os

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


# ---------------------------------------------------------------- the recorded trees (tests/golden/gbdt_trees.json)
GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gbdt_trees.json")
GOLDEN_MODES = {"sort": dict(level="sort"), "partition": dict(level="partition"),
                "subtract": dict(level="partition", subtract=True)}


def small_deep_data():
    """64 rows, 3 features, 8 bins: at depth 6 every tree has levels where some frontier nodes split and
    others are final leaves, the smallest shape that exercises the partition's subset bookkeeping."""
    from mp4x.models.gbdt import quantize
    rng = np.random.default_rng(11)
    X = rng.normal(size=(64, 3))
    y = np.sin(X[:, 0]) + X[:, 1] ** 2 + 0.1 * rng.normal(size=64)
    return quantize(X, 8)[0], y


# name -> (data, B, the trainer's settings)
GOLDEN_CASES = {"a": (model_data, 16, dict(trees=4, depth=3)), "b": (small_deep_data, 8, dict(trees=3, depth=6))}


def golden_trees(case, mode, comm=None, device="cpu", share=(0, 1)):
    """The trees of a golden case as the record holds them (values as ``float.hex()``), from share ``(r,
    p)`` of the rows: the r-th of p ``array_split`` parts."""
    from mp4x.parallel.gbdt import train_gbdt_quantized
    data, B, settings = GOLDEN_CASES[case]
    Bq, y = data()
    rows = np.array_split(np.arange(len(y)), share[1])[share[0]]
    trees = train_gbdt_quantized(comm, torch.from_numpy(Bq[rows].astype(np.uint8)).to(device),
                                 torch.from_numpy(y[rows]).to(device), B, **settings, **GOLDEN_MODES[mode])
    return [dict(feature=t.feature, threshold=t.threshold, left=t.left, right=t.right, value=[v.hex() for v in t.value])
            for t in trees]


def golden_record():
    with open(GOLDEN_PATH) as f:
        return json.load(f)


# ---------------------------------------------------------------- what is refused
# op -> (the *_torch definition, the device_ops wrapper, a good call): the arguments by name, on the CPU
def _good_hist():
    bins, gh, rows, seg = hist_case(40, 3, 16, 2)
    return dict(bins=bins, gh=gh, rows=rows, seg=seg, B=16)


def _good_partition():
    bins, _, rows, seg = hist_case(40, 3, 16, 2)
    z = torch.zeros(2, dtype=torch.int32)
    return dict(bins=bins, rows=rows, seg=seg, feature=z + 1, threshold=z + 7, first_right=z.clone())


OPS = {
    "quantize": ("gbdt_quantize_torch", "gbdt_quantize", lambda: dict(g=torch.ones(8), h=torch.ones(8), sg=3, sh=-2)),
    "histogram": ("gbdt_hist_torch", "gbdt_histogram", _good_hist),
    "split": ("gbdt_split_torch", "gbdt_best_split", lambda: dict(hist=random_hist(2, 3, 4, 1), sg=3, sh=-2, lam=1.0)),
    "partition": ("gbdt_partition_torch", "gbdt_partition", _good_partition),
    "subtract": ("gbdt_hist_subtract_torch", "gbdt_hist_subtract",
                 lambda: dict(parent=random_hist(3, 2, 4, 2), small=random_hist(2, 2, 4, 3),
                              parent_of=torch.tensor([2, 0], dtype=torch.int32))),
}

BOTH = "both forms refuse"
DEVICE = "the wrapper refuses, the definition accepts on the CPU"        # the device's own limits
DEVICE_ONLY = "the wrapper refuses; no such call of the definition on the CPU"


def _like(t, *shape, dtype=None):
    return torch.zeros(*shape, dtype=dtype or t.dtype, device=t.device)


_SHIFTS = {"shift_bool": True, "shift_float": 3.0, "shift_201": 201, "shift_minus_201": -201}
# op -> name -> (the arguments a bad call replaces, given the good call's on its device; who refuses it)
REFUSED = {
    "quantize": {
        **{name: (lambda a, s=s: dict(sg=s), BOTH) for name, s in _SHIFTS.items()},
        "g_float64": (lambda a: dict(g=a["g"].double()), BOTH),
        "h_of_another_length": (lambda a: dict(h=a["h"][:-1].contiguous()), BOTH),
        "g_2d": (lambda a: dict(g=a["g"].view(2, 4)), BOTH),
        "cpu_tensor": (lambda a: dict(h=a["h"].cpu()), DEVICE_ONLY),
        "out_of_the_wrong_dtype": (lambda a: dict(out=_like(a["g"], 8, 2, dtype=torch.int64)), DEVICE_ONLY),
    },
    "histogram": {
        "B_1": (lambda a: dict(B=1), BOTH),
        "B_257": (lambda a: dict(B=257), BOTH),
        "B_true": (lambda a: dict(B=True), BOTH),
        "bins_int32": (lambda a: dict(bins=a["bins"].to(torch.int32)), BOTH),
        "gh_n_by_3": (lambda a: dict(gh=_like(a["gh"], 40, 3)), BOTH),
        "rows_int64": (lambda a: dict(rows=a["rows"].long()), BOTH),
        "seg_int32": (lambda a: dict(seg=a["seg"].to(torch.int32)), BOTH),
        "seg_empty": (lambda a: dict(seg=a["seg"][:0].contiguous()), BOTH),
        "no_features": (lambda a: dict(bins=a["bins"][:, :0].contiguous()), DEVICE),
        "bins_not_contiguous": (lambda a: dict(bins=a["bins"].t().contiguous().t()), DEVICE),
        "table_of_4097_nodes": (lambda a: dict(seg=_like(a["seg"], 4098)), DEVICE),
        "out_of_the_wrong_shape": (lambda a: dict(out=_like(a["seg"], 2, 3, 16, 1)), DEVICE_ONLY),
    },
    "split": {
        **{name: (lambda a, s=s: dict(sh=s), BOTH) for name, s in _SHIFTS.items()},
        "hist_of_rank_3": (lambda a: dict(hist=a["hist"][0]), BOTH),
        "last_dim_3": (lambda a: dict(hist=_like(a["hist"], 2, 3, 4, 3)), BOTH),
        "B_1": (lambda a: dict(hist=a["hist"][:, :, :1].contiguous()), BOTH),
        "B_257": (lambda a: dict(hist=_like(a["hist"], 1, 1, 257, 2)), DEVICE),
    },
    "partition": {
        "feature_int64": (lambda a: dict(feature=a["feature"].long()), BOTH),
        "threshold_of_length_k_plus_1": (lambda a: dict(threshold=_like(a["threshold"], 3)), BOTH),
        "k_2049": (lambda a: dict(seg=_like(a["seg"], 2050), **{x: _like(a[x], 2049) for x in
                                                                ("feature", "threshold", "first_right")}), BOTH),
    },
    "subtract": {
        "small_with_another_F": (lambda a: dict(small=_like(a["small"], 2, 3, 4, 2)), BOTH),
        "parent_of_int64": (lambda a: dict(parent_of=a["parent_of"].long()), BOTH),
        "parent_of_of_the_wrong_length": (lambda a: dict(parent_of=_like(a["parent_of"], 3)), BOTH),
        "no_cells": (lambda a: dict(parent=_like(a["parent"], 3, 0, 4, 2), small=_like(a["small"], 2, 0, 4, 2)),
                     DEVICE),
        "parent_of_4097_nodes": (lambda a: dict(parent=_like(a["parent"], 4097, 2, 4, 2)), DEVICE),
    },
}
REFUSED_ROWS = [(op, name) for op, rows in REFUSED.items() for name in rows]


def refused_call(op, name, device="cpu"):
    """``(definition, wrapper, arguments, who)``: the names of the op's two forms, the bad call's arguments
    on ``device`` and who refuses it."""
    definition, wrapper, good = OPS[op]
    args = {k: v.to(device) if isinstance(v, torch.Tensor) else v for k, v in good().items()}
    change, who = REFUSED[op][name]
    args.update(change(args))
    return definition, wrapper, args, who
