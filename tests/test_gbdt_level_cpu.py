"""The level advance of the fixed-point GBDT (K17) on the CPU: the partition against the sort of the
default level after the trainer's elementwise move, the sibling subtraction against the histogram of the
second children, and the trainer's ``level="partition"`` / ``subtract`` against the default, on 1 and 2
ranks."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import gbdt_cases as cases  # noqa: E402
import gbdt_level_cases as lcases  # noqa: E402
from harness import run_ranks  # noqa: E402
from mp4x.parallel import gbdt  # noqa: E402

CLEAN = [dict(n=111, F=5, k=3), dict(n=111, F=3, k=64), dict(n=60, F=2, k=1, one_node=True, thr=-1),
         dict(n=5000, F=1, k=1, one_node=True, thr=255)]
LOOP = CLEAN[:2] + [dict(n=111, F=2, k=3, bad_rows=True)] + \
    [dict(n=30, F=2, k=4, seg=s, edges=False) for s in cases.HOSTILE.values()]
ids = dict(ids=lambda c: "-".join(f"{k}{v if k != 'seg' else ''}" for k, v in c.items()))


@pytest.mark.parametrize("case", CLEAN, **ids)
def test_partition_equals_the_sorted_level_after_the_elementwise_move(case):
    """Parents are nodes 0 .. k - 1 (node k: no segment), the children of j are k + 1 + 2j and k + 2 + 2j."""
    bins, rows, seg, feature, threshold, first_right = lcases.part_case(**case)
    (n, F), k = bins.shape, seg.numel() - 1
    rows2, seg2 = gbdt.gbdt_partition_torch(bins, rows, seg, feature, threshold, first_right)
    node_of = torch.full((n,), k, dtype=torch.int64)
    for j in range(k):
        node_of[rows[int(seg[j]):int(seg[j + 1])].long()] = j
    feat_of = torch.cat([torch.where((feature >= 0) & (feature < F), feature, -1).long(), torch.full((1,), -1)])
    thr_of = torch.cat([threshold.long(), torch.zeros(1, dtype=torch.int64)])
    b_row = bins.gather(1, feat_of[node_of].clamp(min=0)[:, None])[:, 0].to(torch.int64)         # the trainer's move
    child = k + 1 + 2 * node_of + (b_row > thr_of[node_of]).to(torch.int64)
    node_of = torch.where(feat_of[node_of] >= 0, child, node_of)
    slot_of_node = torch.full((3 * k + 1,), -1, dtype=torch.int64)
    for j in range(k):
        fr = int(first_right[j] != 0)
        slot_of_node[k + 1 + 2 * j + fr], slot_of_node[k + 1 + 2 * j + 1 - fr] = j, k + j
    want_rows, want_seg = gbdt.gbdt_level_rows(node_of, slot_of_node, 2 * k)
    total = int(want_seg[-1])                                     # gbdt_level_rows lists the slotless rows behind
    assert torch.equal(seg2, want_seg) and torch.equal(rows2[:total], want_rows[:total])
    assert bool((rows2[int(seg2[-1]):] == -1).all()) and 0 < int(seg2[-1])


@pytest.mark.parametrize("case", LOOP, **ids)
def test_partition_equals_a_python_loop(case):
    bins, rows, seg, feature, threshold, first_right = lcases.part_case(**case)
    (n, F), k, m = bins.shape, seg.numel() - 1, rows.numel()
    rows2, seg2 = gbdt.gbdt_partition_torch(bins, rows, seg, feature, threshold, first_right)
    c, want = gbdt._clamped_bounds(seg, m), [[] for _ in range(2 * k)]
    for j in range(k):
        for r in rows[c[j]:c[j + 1]].tolist():
            if 0 <= r < n and 0 <= feature[j] < F:
                right = int(bins[r, feature[j]]) > int(threshold[j])
                want[j if right == bool(first_right[j]) else k + j].append(r)
    assert [rows2[int(seg2[j]):int(seg2[j + 1])].tolist() for j in range(2 * k)] == want and int(seg2[0]) == 0
    assert bool((rows2[int(seg2[-1]):] == -1).all())


def test_parent_minus_first_children_is_the_histogram_of_the_second_children():
    bins, gh, rows, seg = cases.hist_case(600, 5, 16, 3, high_bins=True)
    _, _, _, feature, threshold, first_right = lcases.part_case(600, 5, 3, edges=False, thr=8)
    parent = gbdt.gbdt_hist_torch(bins, gh, rows, seg, 16)
    rows2, seg2 = gbdt.gbdt_partition_torch(bins, rows, seg, feature, threshold, first_right)
    children = gbdt.gbdt_hist_torch(bins, gh, rows2, seg2, 16)
    large = gbdt.gbdt_hist_subtract_torch(parent, children[:3], torch.arange(3, dtype=torch.int32))
    assert torch.equal(large, children[3:]) and bool(children[3:].any())
    big = torch.full((1, 1, 2, 2), -2 ** 62)
    wrapped = gbdt.gbdt_hist_subtract_torch(big, -big * 1 + 1, torch.tensor([0, 7], dtype=torch.int32)[:1])
    assert wrapped.flatten().tolist() == [2 ** 63 - 1] * 4                      # -2^62 - (2^62 + 1) wraps
    assert not gbdt.gbdt_hist_subtract_torch(big, torch.zeros(1, 1, 2, 2, dtype=torch.int64),
                                             torch.tensor([1], dtype=torch.int32)).any()


def test_the_next_table_is_the_children_of_the_segments_that_split():
    """Segment 1 of 3 is a final leaf, segment 2 puts its right child first: the partition's host
    bookkeeping alone, against the definition of the partition."""
    nodes, left = [3, 4, 6], [1, 3, -1, 7, -1, -1, 9, -1, -1, -1, -1]           # tree nodes 3 and 6 split
    feature, first_right = [1, -1, 0], [0, 0, 1]
    parents, take, next_nodes = gbdt.next_segments(nodes, left, first_right)
    assert (parents, take, next_nodes) == ([0, 2], [0, 2, 3, 5, 6], [7, 10, 8, 9])
    bins, _, rows, seg = cases.hist_case(60, 2, 16, 3)
    i32 = dict(dtype=torch.int32)
    rows2, seg2 = gbdt.gbdt_partition_torch(bins, rows, seg, torch.tensor(feature, **i32), torch.full((3,), 7, **i32),
                                            torch.tensor(first_right, **i32))
    table = seg2[torch.tensor(take)].tolist()
    kp, s2 = len(parents), seg2.tolist()
    assert table == sorted(table) and table[0] == 0 and table[-1] == s2[-1] and len(set(table)) == 2 * kp + 1
    # segment j of the table holds the rows the definition gives child j: first children, then second ones
    for j, (p, second) in enumerate([(p, 0) for p in parents] + [(p, 3) for p in parents]):
        assert (table[j], table[j + 1]) == (s2[second + p], s2[second + p + 1])
        went_right = bins[rows2[table[j]:table[j + 1]].long(), feature[p]] > 7
        assert bool((went_right == (next_nodes[j] == left[nodes[p]] + 1)).all())
    # the first kp + 1 entries are the table of the first children alone
    assert table[:kp + 1] == [s2[p] for p in parents] + [s2[parents[-1] + 1]]


def _trees(comm, level="sort", subtract=False):
    Bq, y = cases.model_data()
    p, r = (comm.getSlaveNum(), comm.getRank()) if comm is not None else (1, 0)
    rows = np.array_split(np.arange(len(y)), p)[r]
    trees = gbdt.train_gbdt_quantized(comm, torch.from_numpy(Bq[rows].astype(np.uint8)), torch.from_numpy(y[rows]), 16,
                                      trees=4, depth=3, level=level, subtract=subtract)
    return [cases.tree_tuple(t) for t in trees]


def _both(comm):
    return _trees(comm, "partition"), _trees(comm, "partition", True)


def test_partition_and_subtract_grow_the_default_trees_on_one_and_two_ranks():
    default = _trees(None)
    assert _both(None) == (default, default)
    res, _, _ = run_ranks(2, _both, timeout=120)
    assert sorted(res) == [0, 1]
    assert all(r == (default, default) for r in res.values())
    assert any(len(t[0]) > 7 for t in default)                   # deep enough that grandchildren are subtracted


def test_subtract_needs_the_partition_level():
    with pytest.raises(ValueError):
        _trees(None, "sort", True)
