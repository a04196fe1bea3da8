"""The definitions of the GBDT losses (K21, mp4x/parallel/gbdt.py) on the CPU: ``gbdt_grad_torch`` against mpmath at
200 bits under a derived bound, the special rows by value, the absmax and the fused quantise against their
meaning, and the trainer on 2 ranks against 1.

The bound: ``|g - exact| <= 2**-24 |exact| + 2**-50`` and the same for ``h``.  The first term is the one rounding
to float32; the second is 8 float64 ulps of a value of at most 1: ``exp_neg`` is within 1 ulp, and the sum, the
quotient, the difference and the product that follow each add at most one rounding of a value of at most 1 (for
softmax the sum over ``C <= 7`` terms is relative to ``S``, which the quotient divides out)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
mpmath = pytest.importorskip("mpmath")

import gbdt_cases as cases  # noqa: E402
import gbdt_grad_cases as gcases  # noqa: E402
from harness import run_ranks  # noqa: E402
from mp4x.parallel import gbdt  # noqa: E402

mpmath.mp.prec = 200


def _exact(loss, cols, ys):
    """Exact (g, h) per class of one row in mpmath."""
    x = [mpmath.mpf(v) for v in cols]
    if loss == "squared":
        return [(x[0] - mpmath.mpf(ys), mpmath.mpf(1))]
    if loss == "logistic":
        p = 1 / (1 + mpmath.exp(-x[0]))
        return [(p - mpmath.mpf(ys), p * (1 - p))]
    m = max(x)
    e = [mpmath.exp(v - m) for v in x]
    return [(ec / sum(e) - (1 if ys == c else 0), ec / sum(e) * (1 - ec / sum(e))) for c, ec in enumerate(e)]


@pytest.mark.parametrize("loss,C", [("squared", 1), ("logistic", 1), ("softmax", 2), ("softmax", 7)])
def test_the_definition_is_within_one_float32_rounding_of_the_exact_gradient(loss, C):
    pred, y = gcases.margins(loss, 120, C, finite=True)
    g, h = (t.reshape(C, -1) for t in gbdt.gbdt_grad_torch(pred, y, loss))
    cols = pred.reshape(C, -1)
    for r in range(cols.shape[1]):
        label = y[r].item()
        if loss == "softmax" and not 0 <= label < C:
            assert not g[:, r].any() and not h[:, r].any()
            continue
        for c, (ge, he) in enumerate(_exact(loss, cols[:, r].tolist(), label)):
            for got, want in ((g[c, r], ge), (h[c, r], he)):
                if abs(want) >= 2.0 ** 128:                     # squared loss at +-1e300: float32 has no such value
                    assert got.item() == (gcases.INF if want > 0 else -gcases.INF)
                    continue
                assert abs(mpmath.mpf(got.item()) - want) <= abs(want) * 2.0 ** -24 + 2.0 ** -50, (r, c, got, want)


def test_rows_that_are_not_finite_and_labels_out_of_range_by_value():
    x = torch.tensor([gcases.NAN, gcases.INF, -gcases.INF], dtype=torch.float64)
    g, h = gbdt.gbdt_grad_torch(x, torch.zeros(3, dtype=torch.float64), "logistic")
    assert g[0].isnan() and h[0].isnan() and g[1:].tolist() == [1.0, 0.0] and h[1:].tolist() == [0.0, 0.0]
    pred = torch.tensor([[0.0, gcases.NAN, 1.0, gcases.INF, 2.0], [0.0, 1.0, gcases.INF, 1.0, -gcases.INF]],
                        dtype=torch.float64)
    g, h = gbdt.gbdt_grad_torch(pred, torch.tensor([2, 0, 1, -1, 0]), "softmax")
    assert g[:, 0].tolist() == [0.0, 0.0] and h[:, 3].tolist() == [0.0, 0.0]            # labels 2 and -1: ignored
    assert g[:, 1:3].isnan().all() and h[:, 1:3].isnan().all()                          # a NaN, a +inf margin
    assert g[:, 4].tolist() == [0.0, 0.0] and h[:, 4].tolist() == [0.0, 0.0]            # -inf: p = (1, 0), label 0


@pytest.mark.parametrize("loss,C", [("squared", 1), ("logistic", 1), ("softmax", 3)])
def test_absmax_and_the_fused_quantise_mean_what_they_say(loss, C):
    for finite in (True, False):
        pred, y = gcases.margins(loss, 60, C, finite=finite)
        g, h = (t.reshape(C, -1) for t in gbdt.gbdt_grad_torch(pred, y, loss))
        want = torch.stack([g.abs().max(dim=1).values, h.abs().max(dim=1).values], dim=1)
        assert gcases.same_floats(gbdt.gbdt_grad_absmax_torch(pred, y, loss), want)
        for sg, sh in (gcases.shifts(C), gcases.shifts(C, wide=True)):
            got = gbdt.gbdt_grad_quantize_torch(pred, y, loss, sg, sh)
            s = torch.stack([sg, sh]).clamp(-200, 200).tolist()
            assert got.dtype == torch.int32 and all(
                torch.equal(got[c], gbdt.gbdt_quantize_torch(g[c], h[c], s[0][c], s[1][c])) for c in range(C))
    empty = pred[..., :0].contiguous()
    assert gbdt.gbdt_grad_absmax_torch(empty, y[:0], loss).tolist() == [[0.0, 0.0]] * C


def _grown(comm, loss):
    bins, cls = gcases.class_data()
    p, r = (comm.getSlaveNum(), comm.getRank()) if comm is not None else (1, 0)
    rows = torch.from_numpy(np.array_split(np.arange(len(cls)), p)[r])
    y = {"softmax": cls, "logistic": (cls > 0).double(), "squared": torch.from_numpy(cases.model_data()[1])}[loss]
    trees = gbdt.train_gbdt_quantized(comm, bins[rows], y[rows], 16, trees=3, depth=3, loss=loss,
                                      classes=3 if loss == "softmax" else None)
    return [cases.tree_tuple(t) for t in trees]


@pytest.mark.parametrize("loss", ["logistic", "softmax"])
def test_two_ranks_grow_the_trees_of_one_rank(loss):
    one = _grown(None, loss)
    res, _, _ = run_ranks(2, _grown, args=(loss,), timeout=120)
    assert len(one) == (9 if loss == "softmax" else 3) and len(one[0][4]) > 1
    assert sorted(res) == [0, 1] and all(trees == one for trees in res.values())


def test_softmax_rounds_lower_the_cross_entropy_and_squared_grows_the_defaults_trees():
    bins, cls = gcases.class_data()
    trees = gbdt.train_gbdt_quantized(None, bins, cls, 16, trees=3, depth=3, loss="softmax", classes=3)

    def entropy(rounds):
        margins = gbdt.predict_gbdt(trees[:3 * rounds], bins, classes=3)
        return float(-torch.log_softmax(margins, dim=0).gather(0, cls[None, :]).mean())
    assert entropy(3) < entropy(1) < float(np.log(3))
    y = torch.from_numpy(cases.model_data()[1])
    for mode in (dict(), dict(level="partition", update="walk")):
        fused = gbdt.train_gbdt_fused(None, bins, y, 16, "squared", trees=3, depth=3, **mode)
        default = gbdt.train_gbdt_quantized(None, bins, y, 16, trees=3, depth=3, **mode)
        assert [cases.tree_tuple(t) for t in fused] == [cases.tree_tuple(t) for t in default]
