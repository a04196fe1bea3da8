"""train_gbdt_quantized on GPU tensors against the CPU run on the same data, Tree for Tree, without a
communicator and on a one-rank one; and one quantise -> histogram -> split step recorded by
``comm.device.capture`` and replayed on fresh gradients against the eager result."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import gbdt_cases as cases  # noqa: E402
from spawn_ranks import run_spawn  # noqa: E402

pytestmark = pytest.mark.gpu


def _train(comm, device):
    from mp4x.parallel.gbdt import train_gbdt_quantized
    Bq, y = cases.model_data()
    trees = train_gbdt_quantized(comm, torch.from_numpy(Bq.astype(np.uint8)).to(device), torch.from_numpy(y).to(device),
                                 16, trees=4, depth=3)
    return [cases.tree_tuple(t) for t in trees]


def _captured(comm):
    from mp4x.ops import device_ops
    from mp4x.parallel import gbdt
    Bq, _ = cases.model_data()
    bins = torch.from_numpy(Bq.astype(np.uint8)).cuda()
    n, B, sg, sh = bins.shape[0], 16, 27, 29
    gen = torch.Generator().manual_seed(11)
    node = torch.randint(0, 3, (n,), generator=gen).cuda()
    rows, seg = gbdt.gbdt_level_rows(node, torch.tensor([0, 1, -1]).cuda(), 2)
    g, h = torch.zeros(n, device="cuda"), torch.ones(n, device="cuda")
    gh = torch.zeros(n, 2, dtype=torch.int32, device="cuda")
    hist = torch.zeros(2, bins.shape[1], B, 2, dtype=torch.int64, device="cuda")
    best = device_ops.GbdtSplit(*(torch.zeros(2, dtype=dt, device="cuda") for dt in
                                  (torch.float64, torch.int32, torch.int32) + (torch.int64,) * 4))

    def step():
        device_ops.gbdt_quantize(g, h, sg, sh, out=gh)
        device_ops.gbdt_histogram(bins, gh, rows, seg, B, out=hist)
        device_ops.gbdt_best_split(hist, sg, sh, 1.0, out=best)

    g.copy_(torch.randn(n, generator=gen))
    graph = comm.device.capture(step)
    same = []
    for _ in range(3):
        g.copy_(torch.randn(n, generator=gen) * 3)
        graph.replay()
        torch.cuda.synchronize()
        replayed = [hist.clone()] + [t.clone() for t in best]
        step()
        torch.cuda.synchronize()
        same.append(all(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a,
                                    b.view(torch.int64) if b.dtype == torch.float64 else b)
                        for a, b in zip(replayed, [hist] + list(best))))
        want = gbdt.gbdt_hist_torch(bins.cpu(), gbdt.gbdt_quantize_torch(g.cpu(), h.cpu(), sg, sh), rows.cpu(), seg.cpu(), B)
        same.append(torch.equal(hist.cpu(), want) and int(best.feature[0]) >= 0)
    return same, _train(comm, "cuda")


def test_gpu_trees_equal_cpu_trees_and_a_captured_level_replays_exactly():
    cpu = _train(None, "cpu")
    assert _train(None, "cuda") == cpu
    res = run_spawn(1, _captured)
    same, trees = res[0]
    assert len(same) == 6 and all(same), same
    assert trees == cpu
