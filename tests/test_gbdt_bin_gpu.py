"""The GBDT binning kernel (csrc/kernels/gbdt_bin.hip) against the CPU definition of mp4x/parallel/gbdt.py, bit
for bit, twice into ``bins`` with sentinel guards on either side: gbdt_bin_cases.CASES (rows around one and two
4096-row tiles, F around one and two 64-feature groups, E on both sides of a step count and at the cap, unsorted
and NaN edges, hostile counts) and the edge-case table of the CPU file."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import gbdt_bin_cases as bcases  # noqa: E402
import gbdt_cases as cases  # noqa: E402
from mp4x.parallel import gbdt  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", bcases.CASES + list(bcases.TABLE), ids=str)
def test_kernel_equals_the_definition(case):
    if isinstance(case, str):
        X, edges, cnt, missing, want = bcases.table_case(case)
    else:
        X, edges, cnt = bcases.bin_case(*case)
        missing = 255 if case[2] % 2 else 200
        want = gbdt.gbdt_bin_torch(X, edges, cnt, missing)
    for _ in range(2):
        buf, out = cases.guarded(tuple(X.shape), torch.uint8, "cuda")
        assert gbdt.gbdt_bin_torch(X.cuda(), edges.cuda(), cnt.cuda(), missing, out=out) is out
        torch.cuda.synchronize()
        assert cases.guards_intact(buf) and torch.equal(out.cpu(), want)


def test_fit_bins_and_the_trainer_on_the_gpu_equal_the_cpu():
    rng = np.random.default_rng(5)
    X = rng.normal(size=(900, 5)).astype(np.float32)
    X[::17, 2] = np.nan
    y = torch.from_numpy(np.sin(X[:, 0]) + X[:, 1] ** 2)
    X, B = torch.from_numpy(X), 16
    want = gbdt.fit_bins(None, X, B)
    got = gbdt.fit_bins(None, X.cuda(), B)
    assert all(g.is_cuda and g.dtype == w.dtype and torch.equal(g.cpu().view(torch.uint8), w.view(torch.uint8))
               for g, w in zip(got, want))
    trees = gbdt.train_gbdt_quantized(None, want[0], y, B, trees=3, depth=3, level="partition")
    grown = gbdt.train_gbdt_quantized(None, got[0], y.cuda(), B, trees=3, depth=3, level="partition")
    assert len(trees[0].value) > 1 and [cases.tree_tuple(t) for t in grown] == [cases.tree_tuple(t) for t in trees]


@pytest.mark.parametrize("name,change", [
    ("cpu_tensor", lambda a: dict(edges=a["edges"].cpu())),
    ("E_256", lambda a: dict(edges=torch.zeros(3, 256, device="cuda"))),
    ("X_not_contiguous", lambda a: dict(X=a["X"].t().contiguous().t())),
    ("cnt_int64", lambda a: dict(cnt=a["cnt"].long())),
])
def test_the_wrapper_refuses(name, change):
    from mp4x.ops import device_ops
    args = dict(zip(("X", "edges", "cnt"), (t.cuda() for t in bcases.bin_case(9, 3, 5, torch.float32))))
    args.update(change(args))
    with pytest.raises(ValueError):
        device_ops.gbdt_bin(**args)
