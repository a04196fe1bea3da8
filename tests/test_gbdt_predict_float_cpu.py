"""The definition of the GBDT walk over float features (K20) on the CPU: ``gbdt_predict_float_torch`` over
``float_forest``'s keys against bin-then-walk (``gbdt_bin_torch``, then ``gbdt_predict_torch``), bit for bit in
``pred`` and ``leaf``; ``float_forest``'s refusals; ``predict_gbdt`` with and without ``edges=``.  No GPU."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import gbdt_predict_cases as pcases  # noqa: E402
import gbdt_predict_float_cases as fcases  # noqa: E402
from mp4x.parallel import gbdt  # noqa: E402


@pytest.mark.parametrize("hand", [False, True], ids=["gbdt_edges", "hand_made"])
@pytest.mark.parametrize("dtype", fcases.DTYPES, ids=str)
@pytest.mark.parametrize("kind", pcases.FORESTS)
def test_float_walk_equals_bin_then_walk(kind, dtype, hand):
    X, init, forest, edges, cnt = fcases.case(kind, 400, 3, dtype, hand)
    assert X.isnan().any() and X.isinf().any() and (X == 0).any()
    want, want_leaf = gbdt.gbdt_predict_torch(gbdt.gbdt_bin_torch(X, edges, cnt), forest, init=init, leaves=True)
    pred, leaf = gbdt.gbdt_predict_float_torch(X, gbdt.float_forest(forest, edges, cnt), init=init, leaves=True)
    assert torch.equal(leaf, want_leaf)
    assert torch.equal(pred.view(torch.int64), want.view(torch.int64))


@pytest.mark.parametrize("name,edges,cnt,key", [
    ("nan_inside", [[1.0, math.nan, 3.0]], [3], None),
    ("descending_inside", [[1.0, 3.0, 2.0]], [3], None),
    ("both_past_cnt", [[1.0, math.nan, 0.0]], [1], 0xfffffffe),
    ("both_in_a_feature_no_node_names", [[1.0, 2.0, 3.0], [math.nan, 2.0, 1.0]], [3, 3], 0xc0000000),
])
def test_float_forest_refuses_edges_that_break_the_equivalence(name, edges, cnt, key):
    """The root names feature 0 and bin threshold 1; ``key`` is its K where the edges are taken (2.0 has the bits
    0x40000000), None where they are refused."""
    forest = gbdt.GbdtForest(torch.tensor([[0, 1, 1, 2], [-1, -1, -1, -1], [-1, -1, -1, -1]], dtype=torch.int32),
                             torch.zeros(3, dtype=torch.float64), torch.tensor([0, 3], dtype=torch.int32), 1)
    args = (forest, torch.tensor(edges, dtype=torch.float32), torch.tensor(cnt, dtype=torch.int32))
    if key is None:
        with pytest.raises(ValueError):
            gbdt.float_forest(*args)
    else:
        assert int(gbdt.float_forest(*args).nodes[0, 1]) & 0xffffffff == key


def test_predict_gbdt_with_edges_equals_the_default_on_the_bins():
    rng = np.random.default_rng(5)
    X = rng.normal(size=(300, 5)).astype(np.float32)
    X[::17, 2] = np.nan
    y, X = torch.from_numpy(np.sin(X[:, 0]) + X[:, 1] ** 2), torch.from_numpy(X)
    bins, edges, cnt = gbdt.fit_bins(None, X, 16)
    trees = gbdt.train_gbdt_quantized(None, bins, y, 16, trees=3, depth=3)
    init = torch.linspace(-1, 1, 300, dtype=torch.float64)
    default = gbdt.predict_gbdt(trees, bins, init)
    assert len(trees[0].value) > 1
    assert torch.equal(default.view(torch.int64), gbdt.gbdt_predict_torch(bins, gbdt.pack_forest(trees), init=init).view(torch.int64))
    assert torch.equal(default.view(torch.int64), gbdt.predict_gbdt(trees, X, init, edges=(edges, cnt)).view(torch.int64))
