"""The definition of the GBDT forest walk (K18) on the CPU: ``gbdt_predict_torch`` against
``Tree.predict_bins`` summed in tree order, bit for bit, ``pack_forest``'s refusals, the trainer's
``update="walk"`` and the limit the native header shares.  No GPU."""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import gbdt_cases as cases  # noqa: E402
import gbdt_predict_cases as pcases  # noqa: E402
from mp4x.models.gbdt import Tree  # noqa: E402
from mp4x.ops import gbdt_args  # noqa: E402
from mp4x.parallel import gbdt  # noqa: E402


def _golden(case):
    """The recorded trees of a golden case and its data."""
    trees = [Tree(t["feature"], t["threshold"], t["left"], t["right"], [float.fromhex(v) for v in t["value"]])
             for t in cases.golden_record()[case]["partition"]["trees"]]
    return trees, cases.GOLDEN_CASES[case][0]()[0]


@pytest.mark.parametrize("case", ["a", "b"])
def test_definition_equals_predict_bins_summed_in_tree_order(case):
    trees, Bq = _golden(case)
    want = np.zeros(len(Bq))
    for t in trees:
        want += t.predict_bins(Bq)
    forest = gbdt.pack_forest(trees)
    pred, leaf = gbdt.gbdt_predict_torch(torch.from_numpy(Bq.astype(np.uint8)), forest, leaves=True)
    assert forest.steps == cases.GOLDEN_CASES[case][2]["depth"] and forest.tree_off.tolist()[0] == 0
    assert np.array_equal(pred.numpy().view(np.int64), want.view(np.int64))
    for t, tree in enumerate(trees):                    # a direct walk
        for r in range(0, len(Bq), 7):
            j = 0
            while tree.left[j] >= 0:
                j = tree.left[j] if Bq[r, tree.feature[j]] <= tree.threshold[j] else tree.right[j]
            assert leaf[r, t] == j


@pytest.mark.parametrize("kind", pcases.FORESTS)
def test_definition_on_any_bits_stays_inside_the_forest(kind):
    bins, init = pcases.rows_case(40, 3)
    f = pcases.forest(kind, 3)
    pred, leaf = gbdt.gbdt_predict_torch(bins, f, init=init, leaves=True)
    T, o = f.tree_off.numel() - 1, gbdt._clamped_bounds(f.tree_off, f.value.numel())
    want = init.clone()
    for t in range(T):
        size = o[t + 1] - o[t]
        assert bool(((leaf[:, t] >= 0) & (leaf[:, t] < size)).all() if size else (leaf[:, t] == -1).all())
        if size:
            want = want + f.value[o[t] + leaf[:, t].long()]
    assert torch.equal(pred.view(torch.int64), want.view(torch.int64))


def test_no_trees_return_init_bit_for_bit():
    init = torch.tensor([-0.0, 5e-324, 1.5], dtype=torch.float64)
    pred = gbdt.gbdt_predict_torch(torch.zeros(3, 2, dtype=torch.uint8), gbdt.pack_forest([]), init=init)
    assert torch.equal(pred.view(torch.int64), init.view(torch.int64)) and pred.data_ptr() != init.data_ptr()


def _chain(edges):
    return Tree([0] * edges + [-1], [3] * edges + [-1], list(range(1, edges + 1)) + [-1],
                list(range(1, edges + 1)) + [-1], [0.5] * (edges + 1))


@pytest.mark.parametrize("name,tree", [
    ("cycle", Tree([0, 0, -1], [1, 1, -1], [1, 0, -1], [2, 2, -1], [0.0] * 3)),
    ("child_out_of_range", Tree([0, -1, -1], [1, -1, -1], [1, -1, -1], [3, -1, -1], [0.0] * 3)),
    ("path_of_65_edges", _chain(65)),
])
def test_pack_forest_refuses(name, tree):
    with pytest.raises(ValueError):
        gbdt.pack_forest([_chain(2), tree])


def test_pack_forest_takes_a_path_of_64_edges_and_the_header_states_the_limit():
    assert gbdt.pack_forest([_chain(64)]).steps == 64 == gbdt_args.MAX_STEPS
    header = os.path.join(os.path.dirname(cases.GOLDEN_PATH), "..", "..", "csrc", "kernels", "gbdt_walk_map.hpp")
    with open(header) as f:
        assert int(re.search(r"^constexpr int kMaxSteps = (\d+);", f.read(), re.M).group(1)) == gbdt_args.MAX_STEPS


@pytest.mark.parametrize("case", ["a", "b"])
def test_update_walk_grows_the_trees_of_the_partition_level(case):
    data, B, settings = cases.GOLDEN_CASES[case]
    Bq, y = data()
    grown = gbdt.train_gbdt_quantized(None, torch.from_numpy(Bq.astype(np.uint8)), torch.from_numpy(y), B, **settings,
                                      level="partition", update="walk")
    got = [dict(feature=t.feature, threshold=t.threshold, left=t.left, right=t.right, value=[v.hex() for v in t.value])
           for t in grown]
    assert got == cases.golden_record()[case]["partition"]["trees"]


def test_update_walk_needs_the_partition_level():
    bins, y = torch.zeros(4, 1, dtype=torch.uint8), torch.zeros(4, dtype=torch.float64)
    with pytest.raises(ValueError):
        gbdt.train_gbdt_quantized(None, bins, y, 4, update="walk")
    with pytest.raises(ValueError):
        gbdt.train_gbdt_quantized(None, bins, y, 4, level="partition", update="leaves")
