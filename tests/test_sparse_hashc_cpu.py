"""The canonical hash reduce-by-key (K5c) on the CPU: ``canonical_rbk_torch`` (the definition in
torch / numpy and the CPU path of ``keyOrder="table"``) against the plain-Python reference
(tests/sparse_hash_ref.py) and against the sort twin's values; its invariance under row
permutations; the -1 run last; and the public option over gloo ranks: a bad ``keyOrder`` is refused
before the call counts, "ascending" is the call without the argument bit for bit, "table" is the
same set of pairs, identical on every rank and call.  No GPU."""
import pytest

torch = pytest.importorskip("torch")

import sparse_hash_ref as ref  # noqa: E402
from harness import run_ranks  # noqa: E402
from mp4x import Operators  # noqa: E402
from mp4x.operators import DType, for_dtype  # noqa: E402
from mp4x.parallel import sparse  # noqa: E402

SUM = for_dtype(Operators.Float.SUM, DType.F32)


def _cases():
    g = torch.Generator().manual_seed(23)
    out = []
    for n, dim, nk in ((1, 1, 1), (1000, 3, 50), (700, 4, 700), (3000, 2, 900)):
        keys = torch.randint(0, nk, (n,), generator=g) * 7919 - 123456          # negative keys among them
        rows = torch.randint(-50, 50, (n, dim), generator=g).float()
        out.append((keys, rows))
    keys = torch.tensor(ref.keys_with_homes(1024, 1016, 1023, 300))             # the probes wrap round
    out.append((keys[torch.randint(0, 300, (500,), generator=g)], torch.randint(-9, 9, (500, 3), generator=g).float()))
    keys = torch.randint(-(1 << 62), 1 << 62, (400,), generator=g) * 2          # sparse 64-bit ids
    keys[::7] = -1
    out.append((keys, torch.randint(-9, 9, (400, 2), generator=g).float()))
    return out


@pytest.mark.parametrize("case", range(6))
def test_canonical_rbk_torch_is_the_plain_python_definition(case):
    keys, rows = _cases()[case]
    k, v, c = sparse.canonical_rbk_torch(keys, rows, SUM)
    rk, rv, rc = ref.canonical_rbk(keys.tolist(), rows.tolist(), lambda a, b: a + b)
    assert k.tolist() == rk and c.tolist() == rc
    assert v.tolist() == rv                                  # integer-valued rows: exact
    # the sort twin's values, reordered
    sk, sv, sc = sparse._rbk_cpu(keys, rows, SUM)
    o = torch.argsort(k)
    assert torch.equal(k[o], sk) and torch.equal(v[o], sv) and torch.equal(c[o], sc)


def test_the_order_is_the_table_not_the_row_order():
    keys, rows = _cases()[3]
    want = sparse.canonical_rbk_torch(keys, rows, SUM)
    assert want[0].tolist() != sorted(want[0].tolist())      # not the ascending order by accident
    g = torch.Generator().manual_seed(5)
    for _ in range(20):
        perm = torch.randperm(keys.numel(), generator=g)
        got = sparse.canonical_rbk_torch(keys[perm], rows[perm], SUM)
        assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_the_run_of_key_minus_one_comes_last():
    keys = torch.tensor([5, -1, 5, 9, -1, -1, -2])
    rows = torch.arange(7).float().view(7, 1).repeat(1, 2)
    k, v, c = sparse.canonical_rbk_torch(keys, rows, SUM)
    assert k.tolist() == ref.canonical_order(keys.tolist()) and k[-1] == -1 and sorted(k.tolist()) == [-2, -1, 5, 9]
    assert c[-1] == 3 and v[-1].tolist() == [10.0, 10.0]
    k, v, c = sparse.canonical_rbk_torch(torch.full((5,), -1), torch.ones(5, 4), SUM)
    assert k.tolist() == [-1] and c.tolist() == [5] and v.tolist() == [[5.0] * 4]
    k, v, c = sparse.canonical_rbk_torch(torch.empty(0, dtype=torch.int64), torch.empty(0, 4), SUM)
    assert k.numel() == 0 and v.shape == (0, 4) and c.numel() == 0


def test_reduce_by_key_takes_the_table_order_when_asked(monkeypatch):
    keys, rows = _cases()[1]
    want = sparse.canonical_rbk_torch(keys, rows, SUM)
    asc = sparse._reduce_by_key(keys, rows, SUM)
    assert asc[0].tolist() == sorted(set(keys.tolist()))
    assert all(torch.equal(a, b) for a, b in zip(sparse._reduce_by_key(keys, rows, SUM, key_order="table"), want))
    monkeypatch.setattr(sparse, "RBK_MODE", "hashc")         # MP4X_SPARSE_RBK=hashc: the same, process-wide
    assert all(torch.equal(a, b) for a, b in zip(sparse._reduce_by_key(keys, rows, SUM), want))
    assert sparse._reduce_by_key(keys, None, None)[0].tolist() == sorted(set(keys.tolist()))   # keys only: as before
    with pytest.raises(ValueError):
        sparse.check_key_order("descending")


def _key_order_ranks(comm):
    from mp4x import Mp4jException
    # CPU ranks on every host: a forked rank cannot initialise a GPU its parent has looked at
    torch.cuda.is_available = lambda: False
    r = comm.getRank()
    g = torch.Generator().manual_seed(40 + r)
    keys = (torch.randperm(600, generator=g)[:400] - 100) * 1_000_003           # overlapping, some negative
    vals = torch.randint(-8, 8, (400, 3), generator=g).float()
    calls = dict(comm.stats["calls"])
    for bad in ("descending", None, "TABLE"):
        for call in (lambda: comm.allreduceSparse(keys, vals, Operators.Float.SUM, keyOrder=bad),
                     lambda: comm.reduceSparse(keys, vals, Operators.Float.SUM, 0, keyOrder=bad)):
            try:
                call()
                raise AssertionError(f"keyOrder={bad!r} was not refused")
            except Mp4jException:
                pass
    assert dict(comm.stats["calls"]) == calls                # refused before the call counts
    k0, v0 = comm.allreduceSparse(keys, vals, Operators.Float.SUM)
    k1, v1 = comm.allreduceSparse(keys, vals, Operators.Float.SUM, keyOrder="ascending")
    assert torch.equal(k0, k1) and torch.equal(v0, v1)
    k2, v2 = comm.allreduceSparse(keys, vals, Operators.Float.SUM, keyOrder="table")
    k3, v3 = comm.allreduceSparse(keys, vals, Operators.Float.SUM, keyOrder="table")
    assert torch.equal(k2, k3) and torch.equal(v2, v3)
    o0, o2 = torch.argsort(k0), torch.argsort(k2)
    assert torch.equal(k0[o0], k2[o2]) and torch.equal(v0[o0], v2[o2])
    rk, rv = comm.reduceSparse(keys, vals, Operators.Float.SUM, 0, keyOrder="table")
    if r == 0:
        assert torch.equal(rk, k0[o0]) and torch.equal(rv, v0[o0])
    return k0.tolist(), k2.tolist(), v2.tolist()


def test_key_order_through_the_public_api():
    res, _, _ = run_ranks(2, _key_order_ranks, timeout=120)
    (a0, t0, v0), (a1, t1, v1) = res[0], res[1]
    assert a0 == a1 and t0 == t1 and v0 == v1                # the same tensors on both ranks
    assert t0 != a0 and sorted(t0) == sorted(a0)             # and the table order is another order
