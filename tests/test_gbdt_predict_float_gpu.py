"""The GBDT walk kernel over float features (csrc/kernels/gbdt_predict_float.hip) against the CPU definition of
mp4x/parallel/gbdt.py, bit for bit: every case of gbdt_predict_float_cases.CASES runs twice into ``pred`` and
``leaf`` with sentinel guards on either side.  Rows: one, one tile - 1, one tile + 1 and two tiles + 17, the tile
being the header's for that F (1024 rows at F = 1 and 3, 512 at 13, 256 at 43, the largest F staged in LDS, 1024
at 44, the smallest F read from global memory)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import gbdt_cases as cases  # noqa: E402
import gbdt_predict_float_cases as fcases  # noqa: E402
from mp4x.parallel import gbdt  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind,n,F,dtype,init_mode", fcases.CASES, ids=str)
def test_kernel_equals_the_definition(kind, n, F, dtype, init_mode):
    X, init, forest, edges, cnt = fcases.case(kind, n, F, dtype)
    forest = gbdt.float_forest(forest, edges, cnt)
    T = forest.tree_off.numel() - 1
    want, want_leaf = gbdt.gbdt_predict_float_torch(X, forest, init=None if init_mode == "none" else init, leaves=True)
    dev = gbdt.GbdtForest(*(t.cuda() for t in forest[:3]), forest.steps)
    runs = []
    for _ in range(2):
        (pbuf, pred), (lbuf, leaf) = cases.guarded((n,), torch.float64, "cuda"), cases.guarded((n, T), torch.int32, "cuda")
        given = {"none": None, "given": init.cuda(), "alias": pred.copy_(init)}[init_mode]
        gbdt.gbdt_predict_float_torch(X.cuda(), dev, init=given, leaves=True, out=(pred, leaf))
        torch.cuda.synchronize()
        assert cases.guards_intact(pbuf) and cases.guards_intact(lbuf)
        runs.append((pred.cpu().view(torch.int64), leaf.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][1], want_leaf)
    assert torch.equal(runs[0][0], want.view(torch.int64))


def test_predict_gbdt_with_edges_on_the_gpu_equals_the_cpu_on_the_bins():
    rng = np.random.default_rng(5)
    X = rng.normal(size=(900, 5)).astype(np.float32)
    X[::17, 2] = np.nan
    y, X = torch.from_numpy(np.sin(X[:, 0]) + X[:, 1] ** 2), torch.from_numpy(X)
    bins, edges, cnt = gbdt.fit_bins(None, X, 16)
    trees = gbdt.train_gbdt_quantized(None, bins, y, 16, trees=3, depth=3)
    got = gbdt.predict_gbdt(trees, X.cuda(), edges=(edges, cnt))
    assert got.is_cuda and torch.equal(got.cpu().view(torch.int64), gbdt.predict_gbdt(trees, bins).view(torch.int64))


@pytest.mark.parametrize("name,change", [
    ("cpu_tensor", lambda a: dict(value=a["value"].cpu())),
    ("steps_65", lambda a: dict(steps=65)),
    ("X_not_contiguous", lambda a: dict(X=a["X"].t().contiguous().t())),
    ("X_float64", lambda a: dict(X=a["X"].double())),
])
def test_the_wrapper_refuses(name, change):
    from mp4x.ops import device_ops
    X, _, f, edges, cnt = fcases.case("cross_a_chunk", 9, 3, torch.float32)
    f = gbdt.float_forest(f, edges, cnt)
    args = dict(X=X.cuda(), nodes=f.nodes.cuda(), value=f.value.cuda(), tree_off=f.tree_off.cuda(), steps=f.steps)
    args.update(change(args))
    with pytest.raises(ValueError):
        device_ops.gbdt_predict_float(**args)
