"""train_gbdt_quantized with ``level="partition"`` and ``subtract`` on GPU tensors against the CPU default,
Tree for Tree; and one partition -> histogram of the first children -> subtract -> split step recorded
by ``comm.device.capture`` on a one-rank communicator and replayed on fresh gradients and fresh split
inputs against the eager result."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import gbdt_cases as cases  # noqa: E402
from spawn_ranks import run_spawn  # noqa: E402

pytestmark = pytest.mark.gpu


def _train(device, **options):
    from mp4x.parallel.gbdt import train_gbdt_quantized
    Bq, y = cases.model_data()
    trees = train_gbdt_quantized(None, torch.from_numpy(Bq.astype(np.uint8)).to(device), torch.from_numpy(y).to(device),
                                 16, trees=4, depth=3, **options)
    return [cases.tree_tuple(t) for t in trees]


def test_gpu_trees_of_both_options_equal_the_cpu_default():
    cpu = _train("cpu")
    assert _train("cuda", level="partition") == cpu
    assert _train("cuda", level="partition", subtract=True) == cpu


def _captured(comm):
    from mp4x.ops import device_ops
    from mp4x.parallel import gbdt
    Bq, _ = cases.model_data()
    bins = torch.from_numpy(Bq.astype(np.uint8)).cuda()
    (n, F), B, k, sg, sh = bins.shape, 16, 2, 27, 29
    gen = torch.Generator().manual_seed(13)
    rows, seg = torch.randperm(n, generator=gen).to(torch.int32).cuda(), torch.tensor([0, 500, n]).cuda()
    gh = torch.zeros(n, 2, dtype=torch.int32, device="cuda")
    split = torch.zeros(3, k, dtype=torch.int32, device="cuda")                   # feature, threshold, first_right
    parent = torch.zeros(k, F, B, 2, dtype=torch.int64, device="cuda")
    rows2, seg2 = torch.full((n,), -1, dtype=torch.int32, device="cuda"), torch.zeros(2 * k + 1, dtype=torch.int64, device="cuda")
    hist = torch.zeros(2 * k, F, B, 2, dtype=torch.int64, device="cuda")
    parent_of = torch.arange(k, dtype=torch.int32, device="cuda")
    best = device_ops.GbdtSplit(*(torch.zeros(2 * k, dtype=dt, device="cuda") for dt in
                                  (torch.float64, torch.int32, torch.int32) + (torch.int64,) * 4))

    def step():
        device_ops.gbdt_histogram(bins, gh, rows, seg, B, out=parent)
        device_ops.gbdt_partition(bins, rows, seg, split[0], split[1], split[2], out=(rows2, seg2))
        device_ops.gbdt_histogram(bins, gh, rows2, seg2[:k + 1], B, out=hist[:k])
        device_ops.gbdt_hist_subtract(parent, hist[:k], parent_of, out=hist[k:])
        device_ops.gbdt_best_split(hist, sg, sh, 1.0, out=best)

    def fresh():
        gh.copy_(torch.randint(-2 ** 30, 2 ** 30, (n, 2), generator=gen).to(torch.int32))
        gh[:, 1].abs_()
        split.copy_(torch.stack([torch.randint(0, F, (k,), generator=gen), torch.randint(2, 13, (k,), generator=gen),
                                 torch.randint(0, 2, (k,), generator=gen)]).to(torch.int32))

    fresh()
    graph = comm.device.capture(step)
    same = []
    for _ in range(3):
        fresh()
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.clone() for t in (rows2, seg2, hist) + tuple(best)]
        rows2.fill_(-1)
        step()
        torch.cuda.synchronize()
        same.append(all(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a,
                                    b.view(torch.int64) if b.dtype == torch.float64 else b)
                        for a, b in zip(replayed, (rows2, seg2, hist) + tuple(best))))
        want_rows, want_seg = gbdt.gbdt_partition_torch(bins.cpu(), rows.cpu(), seg.cpu(), *split.cpu())
        want = gbdt.gbdt_hist_torch(bins.cpu(), gh.cpu(), want_rows, want_seg, B)     # all 2k children, histogrammed
        same.append(torch.equal(seg2.cpu(), want_seg) and torch.equal(rows2.cpu(), want_rows) and
                    torch.equal(hist.cpu(), want) and 0 < int(want_seg[k]) < int(want_seg[-1]))
    return same


def test_a_captured_partition_subtract_level_replays_exactly():
    same = run_spawn(1, _captured)[0]
    assert len(same) == 6 and all(same), same
