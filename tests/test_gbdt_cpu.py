"""The definitions of the fixed-point GBDT (mp4x/parallel/gbdt.py) on the CPU: the quantiser against
exact rational arithmetic, the histogram against a Python loop and against the float64 sum of the
unquantised values (one rounding a row), the split's tie rules, and the trainer on 3 ranks against 1."""
import math
from fractions import Fraction

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import gbdt_cases as cases  # noqa: E402
from harness import run_ranks  # noqa: E402
from mp4x.parallel import gbdt  # noqa: E402


@pytest.mark.parametrize("maxabs,s", [(1.0, 29), (0.75, 30), (0.5, 30), (3.0, 28), (2.0 ** -40, 69), (0.0, 0),
                                      (float("inf"), 0), (float("nan"), 0)])
def test_the_shift_puts_the_largest_magnitude_below_two_to_the_30(maxabs, s):
    assert gbdt.gbdt_shift(maxabs) == s
    if s:
        assert 2 ** 29 <= maxabs * 2.0 ** s < 2 ** 30


def _q_exact(x, s):
    if math.isnan(x):
        return 0
    if math.isinf(x):
        return cases.QMAX if x > 0 else -cases.QMAX
    return max(-cases.QMAX, min(cases.QMAX, round(Fraction(x) * Fraction(2) ** s)))     # round(Fraction): half to even


def test_quantize_rounds_once_to_even_and_clamps():
    (gv, sg), (hv, sh) = cases.QUANT_G, cases.QUANT_H
    g, h = torch.tensor(gv, dtype=torch.float32), torch.tensor(hv, dtype=torch.float32)
    want = [[_q_exact(a, sg), _q_exact(b, sh)] for a, b in zip(g.tolist(), h.tolist())]
    got = gbdt.gbdt_quantize_torch(g, h, sg, sh)
    assert got.dtype == torch.int32 and got.tolist() == want
    assert [w[0] for w in want[4:8]] == [2, 4, -2, -4] and want[10][0] == cases.QMAX       # the fixture does hit the halves


HIST = [dict(n=111, F=5, B=16, k=3), dict(n=111, F=3, B=2, k=64), dict(n=60, F=2, B=255, k=1, one_node=True),
        dict(n=111, F=2, B=4, k=3, bad_rows=True, high_bins=True), dict(n=40, F=2, B=4, k=3, one_bin=True)] + \
       [dict(n=30, F=2, B=4, k=4, seg=s) for s in cases.HOSTILE.values()]


@pytest.mark.parametrize("case", HIST, ids=lambda c: "-".join(f"{k}{v if k != 'seg' else ''}" for k, v in c.items()))
def test_histogram_equals_a_python_loop(case):
    bins, gh, rows, seg = cases.hist_case(**case)
    B, (n, F), m, k = case["B"], bins.shape, rows.numel(), seg.numel() - 1
    want = np.zeros((k, F, B, 2), dtype=object)
    c = 0
    for j in range(k):
        hi = max(c, min(int(seg[j + 1]), m))
        for r in rows[c:hi].tolist():
            if 0 <= r < n:
                for f in range(F):
                    if bins[r, f] < B:
                        want[j, f, bins[r, f]] += np.array(gh[r].tolist(), dtype=object)
        c = hi
    assert gbdt.gbdt_hist_torch(bins, gh, rows, seg, B).tolist() == want.tolist()


def test_a_quantised_bin_is_within_half_a_step_a_row_of_the_float64_sum():
    gen = torch.Generator().manual_seed(7)
    n, B = 4000, 16
    g, h = torch.randn(n, generator=gen), torch.rand(n, generator=gen)
    bins = torch.randint(0, B, (n, 1), dtype=torch.uint8, generator=gen)
    sg, sh = gbdt.gbdt_shift(float(g.abs().max())), gbdt.gbdt_shift(float(h.abs().max()))
    gh = gbdt.gbdt_quantize_torch(g, h, sg, sh)
    hist = gbdt.gbdt_hist_torch(bins, gh, torch.arange(n, dtype=torch.int32), torch.tensor([0, n]), B)[0, 0]
    for b in range(B):
        sel = bins[:, 0] == b
        cnt = int(sel.sum())
        for col, (x, s) in enumerate(((g, sg), (h, sh))):
            err = abs(int(hist[b, col]) * 2.0 ** -s - math.fsum(x[sel].double().tolist()))
            assert err <= cnt * 2.0 ** (-s - 1), (b, col, err)


@pytest.mark.parametrize("name", sorted(cases.SPLIT))
def test_split_tie_rules_and_nodes_without_a_split(name):
    hist, sg, sh, lam, feature, threshold = cases.SPLIT[name]
    best = gbdt.gbdt_split_torch(hist, sg, sh, lam)
    assert (int(best.feature[0]), int(best.threshold[0])) == (feature, threshold)
    pre = hist[0].cumsum(1)
    f = max(feature, 0)
    assert (int(best.G[0]), int(best.H[0])) == tuple(pre[f, -1].tolist())
    if feature >= 0:
        assert (int(best.GL[0]), int(best.HL[0])) == tuple(pre[f, threshold].tolist()) and float(best.gain[0]) > 1e-12
    else:
        assert (int(best.GL[0]), int(best.HL[0])) == (0, 0) and not float(best.gain[0]) > 1e-12


def _quantized(comm):
    Bq, y = cases.model_data()
    p, r = (comm.getSlaveNum(), comm.getRank()) if comm is not None else (1, 0)
    rows = np.array_split(np.arange(len(y)), p)[r]
    trees = gbdt.train_gbdt_quantized(comm, torch.from_numpy(Bq[rows].astype(np.uint8)), torch.from_numpy(y[rows]), 16,
                                      trees=4, depth=3)
    return [cases.tree_tuple(t) for t in trees]


def test_three_ranks_grow_the_trees_of_one_rank_and_train_gbdt_picks_the_same_splits():
    from mp4x.models.gbdt import train_gbdt
    one = _quantized(None)
    res, _, _ = run_ranks(3, _quantized, timeout=120)
    assert sorted(res) == [0, 1, 2]
    for trees in res.values():
        assert trees == one                                         # values included, bit for bit
    Bq, y = cases.model_data()
    ref = train_gbdt(None, Bq, y, 16, trees=4, depth=3)
    assert [(t[0], t[1]) for t in one] == [(t.feature, t.threshold) for t in ref]
