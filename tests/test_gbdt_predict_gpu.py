"""The GBDT forest walk kernel (csrc/kernels/gbdt_predict.hip) against the CPU definition of
mp4x/parallel/gbdt.py, bit for bit: every case runs twice into ``pred`` and ``leaf`` with sentinel guards on
either side.  A row tile is 1024 rows and a chunk 512 nodes, so the shapes of gbdt_predict_cases.CASES are
one row, one tile - 1, one tile + 1 and two tiles + 17 rows over forests that fit one chunk, cross one, or
start with one tree too large for a chunk, at F = 1, 3, 37 (bins staged in LDS) and 45 (the smallest F whose
bins are read from global memory)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import gbdt_cases as cases  # noqa: E402
import gbdt_predict_cases as pcases  # noqa: E402
from mp4x.parallel import gbdt  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind,n,F,init_mode", pcases.CASES)
def test_kernel_equals_the_definition(kind, n, F, init_mode):
    bins, init = pcases.rows_case(n, F)
    forest = pcases.forest(kind, F)
    T = forest.tree_off.numel() - 1
    want, want_leaf = gbdt.gbdt_predict_torch(bins, forest, init=None if init_mode == "none" else init, leaves=True)
    dev = gbdt.GbdtForest(*(t.cuda() for t in forest[:3]), forest.steps)
    runs = []
    for _ in range(2):
        (pbuf, pred), (lbuf, leaf) = cases.guarded((n,), torch.float64, "cuda"), cases.guarded((n, T), torch.int32, "cuda")
        given = {"none": None, "given": init.cuda(), "alias": pred.copy_(init)}[init_mode]
        gbdt.gbdt_predict_torch(bins.cuda(), dev, init=given, leaves=True, out=(pred, leaf))
        torch.cuda.synchronize()
        assert cases.guards_intact(pbuf) and cases.guards_intact(lbuf)
        runs.append((pred.cpu().view(torch.int64), leaf.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][1], want_leaf)
    assert torch.equal(runs[0][0], want.view(torch.int64))


def test_predict_gbdt_and_update_walk_on_the_gpu_equal_the_cpu():
    data, B, settings = cases.GOLDEN_CASES["b"]
    Bq, y = data()
    bins, yt = torch.from_numpy(Bq.astype(np.uint8)), torch.from_numpy(y)
    trees = gbdt.train_gbdt_quantized(None, bins, yt, B, **settings, level="partition")
    want = gbdt.predict_gbdt(trees, bins)
    got = gbdt.predict_gbdt(trees, bins.cuda())
    assert got.is_cuda and torch.equal(got.cpu().view(torch.int64), want.view(torch.int64))
    grown = gbdt.train_gbdt_quantized(None, bins.cuda(), yt.cuda(), B, **settings, level="partition", update="walk")
    assert [cases.tree_tuple(t) for t in grown] == [cases.tree_tuple(t) for t in trees]


@pytest.mark.parametrize("name,change", [
    ("cpu_tensor", lambda a: dict(value=a["value"].cpu())),
    ("steps_65", lambda a: dict(steps=65)),
    ("nodes_int64", lambda a: dict(nodes=a["nodes"].long())),
    ("no_features", lambda a: dict(bins=a["bins"][:, :0].contiguous())),
])
def test_the_wrapper_refuses(name, change):
    from mp4x.ops import device_ops
    f = pcases.forest("cross_a_chunk", 3)
    args = dict(bins=pcases.rows_case(9, 3)[0].cuda(), nodes=f.nodes.cuda(), value=f.value.cuda(),
                tree_off=f.tree_off.cuda(), steps=f.steps)
    args.update(change(args))
    with pytest.raises(ValueError):
        device_ops.gbdt_predict(**args)
