"""The GBDT level kernels (csrc/kernels/gbdt_level.hip) against the CPU definitions of
mp4x/parallel/gbdt.py, bit for bit: every call runs twice into outputs with sentinel guards on either
side, pre-filled with the sentinel.  kTile is 4096 row slots, so n = 5000 rows of one node cross two
tiles; the offsets scan takes 256 tiles a pass, so 257 * 4096 + 17 row slots take two."""
import pytest

torch = pytest.importorskip("torch")

import gbdt_cases as cases  # noqa: E402
import gbdt_level_cases as lcases  # noqa: E402
from mp4x.parallel import gbdt  # noqa: E402

pytestmark = pytest.mark.gpu
ids = dict(ids=lambda c: "-".join(f"{k}{v if k != 'seg' else ''}" for k, v in c.items()))


def _partition_twice(case_tensors, m, k):
    from mp4x.ops import device_ops
    dev = [t.cuda() for t in case_tensors]
    runs = []
    for _ in range(2):
        (rbuf, rows2), (sbuf, seg2) = cases.guarded((m,), torch.int32, "cuda"), cases.guarded((2 * k + 1,), torch.int64, "cuda")
        device_ops.gbdt_partition(*dev, out=(rows2, seg2))
        torch.cuda.synchronize()
        assert cases.guards_intact(rbuf) and cases.guards_intact(sbuf)
        runs.append((rows2.cpu(), seg2.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    return runs[0]


@pytest.mark.parametrize("case", lcases.PARTITION, **ids)
def test_partition_kernels_equal_the_definition(case):
    tensors = lcases.part_case(**case)
    _, rows, seg = tensors[:3]
    want_rows, want_seg = gbdt.gbdt_partition_torch(*tensors)
    got_rows, got_seg = _partition_twice(tensors, rows.numel(), seg.numel() - 1)
    total = int(want_seg[-1])
    assert torch.equal(got_seg, want_seg)
    assert torch.equal(got_rows[:total], want_rows[:total])
    assert bool((got_rows[total:] == 77).all())                   # the undefined tail is not touched


def test_partition_of_no_row_slots_writes_a_zero_table_only():
    bins, _, seg, feature, threshold, first_right = lcases.part_case(111, 5, 3)
    rows = torch.zeros(0, dtype=torch.int32)
    _, got_seg = _partition_twice((bins, rows, seg, feature, threshold, first_right), 0, 3)
    assert got_seg.tolist() == [0] * 7


@pytest.mark.parametrize("F,B", [(1, 2), (1, 256), (37, 2), (37, 256)])
def test_subtract_kernel_equals_the_definition(F, B):
    from mp4x.ops import device_ops
    parent, small = cases.random_hist(3, F, B, F + B), cases.random_hist(5, F, B, F + B + 1)
    parent[0, 0, 0], small[0, 0, 0] = torch.tensor([-cases.BIG, cases.BIG]), torch.tensor([cases.BIG + 5, -cases.BIG - 5])
    small[4, 0, 1, 0] = -cases.BIG                                # under the out-of-range parent: 0 - x
    parent_of = torch.tensor([0, 2, 2, 1, 3], dtype=torch.int32)   # a repeat, and 3 is outside [0, k)
    want = gbdt.gbdt_hist_subtract_torch(parent, small, parent_of)
    assert want[0, 0, 0].tolist() == [2 ** 63 - 5, -2 ** 63 + 5] and torch.equal(want[4], -small[4])     # it wrapped
    runs = []
    for _ in range(2):
        buf, out = cases.guarded(tuple(small.shape), torch.int64, "cuda")
        device_ops.gbdt_hist_subtract(parent.cuda(), small.cuda(), parent_of.cuda(), out=out)
        torch.cuda.synchronize()
        assert cases.guards_intact(buf)
        runs.append(out.cpu())
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], want)
