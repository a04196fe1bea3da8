"""The definitions of the GBDT feature binning (K19) on the CPU: ``gbdt_bin_torch`` against ``np.searchsorted``,
``models.gbdt.quantize`` and a table of edge cases, ``gbdt_edges`` against a plain sort of the whole column and on
two ranks against one, and what both refuse.  No GPU."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import gbdt_bin_cases as bcases  # noqa: E402
from harness import run_ranks  # noqa: E402
from mp4x.models.gbdt import quantize  # noqa: E402
from mp4x.parallel import gbdt  # noqa: E402


def _bits(t):
    return t.contiguous().view(torch.int32).tolist()


@pytest.mark.parametrize("E,dtype", [(1, torch.float32), (7, torch.float16), (64, torch.bfloat16), (255, torch.float32)])
def test_ascending_edges_give_searchsorted_right_and_quantize(E, dtype):
    gen = torch.Generator().manual_seed(E)
    edges = torch.randn(5, E, generator=gen).to(dtype).to(torch.float32).sort(dim=1).values
    cnt = torch.tensor([E, E // 2, 0, E, 1], dtype=torch.int32)
    special = torch.tensor(bcases.SPECIALS[1:])[:, None].expand(-1, 5)          # all but the NaN
    X = torch.cat([torch.randn(200, 5, generator=gen), edges.t(), special]).to(dtype)   # every edge is a value too
    wide = X.to(torch.float32).numpy()                                          # half types widen exactly
    got = gbdt.gbdt_bin_torch(X, edges, cnt)
    for f in range(5):
        assert np.array_equal(got[:, f].numpy(), np.searchsorted(edges[f, :cnt[f]].numpy(), wide[:, f], side="right"))
    full = gbdt.gbdt_bin_torch(X, edges, torch.full((5,), E, dtype=torch.int32))
    assert np.array_equal(full.numpy(), quantize(wide, E + 1, edges=list(edges.numpy()))[0])


@pytest.mark.parametrize("name", bcases.TABLE)
def test_the_edge_cases(name):
    X, edges, cnt, missing, want = bcases.table_case(name)
    out = torch.empty_like(want)
    assert gbdt.gbdt_bin_torch(X, edges, cnt, missing, out=out) is out and torch.equal(out, want)


@pytest.mark.parametrize("n,B,dtype", [(5, 16, torch.float32), (1, 2, torch.float32), (300, 16, torch.float32),
                                       (257, 64, torch.float16), (1000, 256, torch.float32)])
def test_edges_equal_a_sort_of_the_whole_column(n, B, dtype):
    X = bcases.edges_case(n, dtype)
    bins, edges, cnt = gbdt.fit_bins(None, X, B)
    want_edges, want_cnt = bcases.brute_edges(X, B)
    assert edges.dtype == torch.float32 and cnt.dtype == torch.int32 and cnt.tolist() == want_cnt
    assert _bits(edges) == _bits(torch.tensor(want_edges, dtype=torch.float32))
    assert torch.equal(bins, gbdt.gbdt_bin_torch(X, edges, cnt)) and bool((bins[:, 2] == 255).all())


def _edges_of_a_share(comm, n, B, cut):
    X = bcases.edges_case(n)
    if comm is not None:
        X = X[:cut] if comm.getRank() == 0 else X[cut:]
    edges, cnt = gbdt.gbdt_edges(comm, X, B)
    return _bits(edges), cnt.tolist()


@pytest.mark.parametrize("n,B,cut", [(300, 16, 7), (40, 64, 0)])
def test_two_ranks_give_the_edges_of_one(n, B, cut):
    res, _, _ = run_ranks(2, _edges_of_a_share, args=(n, B, cut), timeout=120)
    assert sorted(res) == [0, 1] and res[0] == res[1] == _edges_of_a_share(None, n, B, cut)


_X, _E, _C = torch.zeros(4, 3), torch.zeros(3, 5), torch.zeros(3, dtype=torch.int32)


@pytest.mark.parametrize("name,args", [
    ("X_float64", (_X.double(), _E, _C, 255)), ("X_1d", (_X[0], _E, _C, 255)), ("edges_float64", (_X, _E.double(), _C, 255)),
    ("edges_of_another_F", (_X, _E[:2], _C, 255)), ("E_256", (_X, torch.zeros(3, 256), _C, 255)),
    ("cnt_int64", (_X, _E, _C.long(), 255)), ("cnt_of_another_F", (_X, _E, _C[:2], 255)),
    ("missing_256", (_X, _E, _C, 256)), ("missing_minus_1", (_X, _E, _C, -1)), ("missing_true", (_X, _E, _C, True)),
])
def test_the_definition_refuses(name, args):
    with pytest.raises(ValueError):
        gbdt.gbdt_bin_torch(*args)


@pytest.mark.parametrize("X,B", [(_X, 1), (_X, 257), (_X, True), (_X, 16.0), (_X.long(), 16)])
def test_edges_refuse_a_bin_count_outside_2_to_256_and_integer_features(X, B):
    with pytest.raises(ValueError):
        gbdt.gbdt_edges(None, X, B)
