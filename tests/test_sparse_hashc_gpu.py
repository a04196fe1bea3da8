"""K5c, the canonical hash reduce-by-key (csrc/kernels/sparse_hash.hip): the output is a function of
the input — the keys in the order of the canonical table (tests/sparse_hash_ref.py: plain Python),
the values and counts of the deterministic sort path (K5) bit for bit for every run length, the
same bytes for every row order and every repeat — on small and odd shapes, negative keys, probes
that wrap round the table, one long cluster, runs of 65 / 100 / 1000 rows, the -1 key, no rows and
rows that are not whole 16-byte vectors; and through the public option (``keyOrder="table"`` /
``MP4X_SPARSE_RBK=hashc``) with two real processes."""
import functools

import pytest

torch = pytest.importorskip("torch")

import sparse_hash_ref as ref  # noqa: E402
from spawn_ranks import run_spawn  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1000, 3, 50), (4096, 16, 4096), (70000, 5, 900)]     # (n, dim, distinct)


def _aligned(k, v, c):
    o = torch.argsort(k)
    return k[o], v[o], c[o]


def _same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8),
                                                                     b.contiguous().view(torch.uint8))


@functools.lru_cache(maxsize=None)
def _int_case(i):
    """(keys, integer-valued int64 rows) on the CPU, shared by the tests (never modified)."""
    n, dim, nk = SHAPES[i]
    g = torch.Generator().manual_seed(7 + i)
    keys = torch.randint(0, nk, (n,), generator=g) * 7919 - 123456             # negative keys among them
    return keys, torch.randint(-50, 50, (n, dim), generator=g)


@functools.lru_cache(maxsize=None)
def _wrap_keys():
    return ref.keys_with_homes(1024, 1016, 1023, 300)         # homes in the last 8 of t = 1024 slots


@functools.lru_cache(maxsize=None)
def _cluster_keys():
    return ref.keys_with_homes(1024, 700, 700, 400, start=(1 << 63) + 1, step=1)   # one home; top bit set


def _signed(keys):
    return [k - (1 << 64) if k >> 63 else k for k in keys]


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_keys_come_in_canonical_table_order(i):
    from mp4x.ops.device_ops import hash_reduce_by_key_canonical
    keys, rows = _int_case(i)
    k, v, c = hash_reduce_by_key_canonical(keys.cuda(), rows.float().cuda(), 0)
    assert k.tolist() == ref.canonical_order(keys.tolist())


def test_order_of_negative_keys_wrapping_probes_and_one_long_cluster():
    from mp4x.ops.device_ops import hash_reduce_by_key_canonical
    g = torch.Generator().manual_seed(31)
    neg = list(dict.fromkeys((-torch.randint(2, 1 << 40, (900,), generator=g)).tolist() +
                             [-(1 << 63), (1 << 63) - 1, 0, -2]))
    wrap, cluster = _wrap_keys(), _signed(_cluster_keys())
    assert len(set(wrap)) == 300 and all(ref.home(k, 1024) >= 1016 for k in wrap)
    assert len(set(cluster)) == 400 and all(ref.home(k, 1024) == 700 for k in cluster)
    table = ref.canonical_table(wrap)
    assert table[0] is not None and table[1015] is None      # the cluster does wrap
    for keys in (neg, wrap, cluster):
        kt = torch.tensor(keys)[torch.randperm(len(keys), generator=g)]
        rows = torch.randint(-9, 9, (len(keys), 4), generator=g).float()
        k, v, c = hash_reduce_by_key_canonical(kt.cuda(), rows.cuda(), 0)
        assert k.tolist() == ref.canonical_order(kt.tolist())
        assert torch.equal(v.cpu(), rows[[kt.tolist().index(x) for x in k.tolist()]]) and bool((c == 1).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.int32, torch.int64])
@pytest.mark.parametrize("op", [0, 1, 2])           # SUM, MAX, MIN
def test_values_and_counts_are_the_sort_paths_on_integer_rows(dtype, op):
    from mp4x.ops.device_ops import hash_reduce_by_key_canonical, reduce_by_key
    for i in range(len(SHAPES)):
        keys, rows = _int_case(i)
        keys, rows = keys.cuda(), rows.to(dtype).cuda()
        hk, hv, hc = _aligned(*hash_reduce_by_key_canonical(keys, rows, op))
        sk, sv, sc = reduce_by_key(keys, rows, op)
        assert torch.equal(hk, sk) and torch.equal(hc, sc)
        assert torch.equal(hv, sv), (dtype, op, i, (hv != sv).sum().item())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64])
def test_values_are_bit_for_bit_the_sort_paths_on_random_floats(dtype):
    from mp4x.ops.device_ops import hash_reduce_by_key_canonical, reduce_by_key
    g = torch.Generator(device="cuda").manual_seed(3)
    for n, dim, nk in ((50_000, 7, 3000), (4096, 16, 512), (3000, 64, 40)):       # the last: runs of ~75 rows
        keys = torch.randint(0, nk, (n,), device="cuda", generator=g) * 1_000_003
        rows = torch.randn(n, dim, device="cuda", generator=g).to(dtype)
        for op in (0, 3):                                                         # SUM, PROD
            hk, hv, hc = _aligned(*hash_reduce_by_key_canonical(keys, rows, op))
            sk, sv, sc = reduce_by_key(keys, rows, op)
            assert torch.equal(hk, sk) and torch.equal(hc, sc)
            assert _same_bytes(hv, sv), (dtype, n, op)


@pytest.mark.parametrize("run", [65, 100, 1000])
@pytest.mark.parametrize("dtype,dim", [(torch.float32, 8), (torch.bfloat16, 5), (torch.float32, 67)])
def test_long_runs_combine_in_input_order(run, dtype, dim):
    """One key repeated ``run`` times among 2000 other rows: its rows combine in ascending input
    index (batches of 64), as in the sort path — the same bits — and the same bytes on every call.
    Rows of whole 16-byte vectors, of 10 bytes, and of more elements (67) than a run has lanes."""
    from mp4x.ops.device_ops import hash_reduce_by_key_canonical, reduce_by_key
    g = torch.Generator().manual_seed(run)
    keys = torch.cat([torch.randint(0, 1500, (2000,), generator=g) * 977, torch.full((run,), 424242)])
    perm = torch.randperm(keys.numel(), generator=g)
    keys = keys[perm].cuda()
    for op in (0, 3):                                                             # SUM, PROD
        rows = torch.randn(keys.numel(), dim, generator=g) if op == 0 else 0.9 + 0.2 * torch.rand(
            keys.numel(), dim, generator=g)                                       # (products stay finite, non-zero)
        rows = rows.to(dtype).cuda()
        first = hash_reduce_by_key_canonical(keys, rows, op)
        hk, hv, hc = _aligned(*first)
        sk, sv, sc = reduce_by_key(keys, rows, op)
        assert torch.equal(hk, sk) and torch.equal(hc, sc) and int(hc.max()) >= run
        assert _same_bytes(hv, sv), (run, dtype, op)
        for _ in range(4):
            again = hash_reduce_by_key_canonical(keys, rows, op)
            assert all(_same_bytes(a, b) for a, b in zip(again, first))


def test_the_result_does_not_depend_on_the_row_order_or_the_run():
    from mp4x.ops.device_ops import hash_reduce_by_key_canonical
    keys, rows = _int_case(3)                                 # 70000 rows, 900 keys: runs of ~78 rows
    keys, rows = keys.cuda(), rows.float().cuda()
    want = hash_reduce_by_key_canonical(keys, rows, 0)
    for _ in range(4):
        assert all(_same_bytes(a, b) for a, b in zip(hash_reduce_by_key_canonical(keys, rows, 0), want))
    g = torch.Generator().manual_seed(9)
    for _ in range(20):
        perm = torch.randperm(keys.numel(), generator=g).cuda()
        got = hash_reduce_by_key_canonical(keys[perm], rows[perm], 0)
        assert all(_same_bytes(a, b) for a, b in zip(got, want))


def test_edges_minus_one_no_rows_and_odd_widths():
    from mp4x.ops.device_ops import hash_reduce_by_key_canonical, reduce_by_key
    keys = torch.tensor([5, -1, 5, 9, -1, -1], device="cuda")
    rows = torch.arange(6, device="cuda").float().view(6, 1).repeat(1, 8)
    k, v, c = hash_reduce_by_key_canonical(keys, rows, 0)
    assert k.tolist() == ref.canonical_order(keys.tolist()) and k.tolist()[-1] == -1      # -1 comes last
    assert c.tolist()[-1] == 3 and v[-1].tolist() == [1.0 + 4 + 5] * 8
    assert sorted(zip(k.tolist(), c.tolist(), v[:, 0].tolist())) == [(-1, 3, 10.0), (5, 2, 2.0), (9, 1, 3.0)]
    k, v, c = hash_reduce_by_key_canonical(torch.full((5,), -1, device="cuda"), torch.ones(5, 4, device="cuda"), 0)
    assert k.tolist() == [-1] and c.tolist() == [5] and v.tolist() == [[5.0] * 4]
    k, v, c = hash_reduce_by_key_canonical(torch.empty(0, dtype=torch.int64, device="cuda"),
                                           torch.empty(0, 4, device="cuda"), 0)
    assert k.numel() == 0 and v.shape == (0, 4) and c.numel() == 0
    g = torch.Generator().manual_seed(13)
    keys = (torch.randint(0, 300, (5000,), generator=g) * 31).cuda()
    for dtype, dim in ((torch.float32, 3), (torch.bfloat16, 5), (torch.float64, 1), (torch.float32, 67)):
        rows = torch.randn(5000, dim, generator=g).to(dtype).cuda()   # 12, 10, 8, 268 bytes: no 16-byte vectors
        hk, hv, hc = _aligned(*hash_reduce_by_key_canonical(keys, rows, 0))
        sk, sv, sc = reduce_by_key(keys, rows, 0)
        assert torch.equal(hk, sk) and torch.equal(hc, sc) and _same_bytes(hv, sv), (dtype, dim)
    one = hash_reduce_by_key_canonical(keys, torch.ones(5000, device="cuda"), 0)            # vals[n]
    assert one[1].shape == one[0].shape and torch.equal(one[1], one[2].float())


def test_reduce_by_key_of_the_map_path_in_hashc_mode(monkeypatch):
    """MP4X_SPARSE_RBK=hashc: sparse ids take K5c (the sort path's pairs, in table order); dense ids
    still take K5d."""
    from mp4x.operators import DType, Operators, for_dtype
    from mp4x.ops import device_ops
    from mp4x.parallel import sparse
    op = for_dtype(Operators.Float.SUM, DType.F32)
    keys, rows = _int_case(1)
    keys, rows = keys.cuda(), rows.float().cuda()
    monkeypatch.setattr(sparse, "RBK_MODE", "sort")
    sk, sv, sc = sparse._reduce_by_key(keys, rows, op)
    tk, tv, tc = sparse._reduce_by_key(keys, rows, op, key_order="table")
    monkeypatch.setattr(sparse, "RBK_MODE", "hashc")
    hk, hv, hc = sparse._reduce_by_key(keys, rows, op)
    assert hk.tolist() == ref.canonical_order(keys.tolist())
    assert torch.equal(hk, tk) and torch.equal(hv, tv) and torch.equal(hc, tc)
    o = torch.argsort(hk)
    assert torch.equal(hk[o], sk) and torch.equal(hv[o], sv) and torch.equal(hc[o], sc)
    calls = []
    real = device_ops.dense_reduce_by_key

    def spy(*a, **k):
        out = real(*a, **k)
        calls.append(out is not None)
        return out
    monkeypatch.setattr(device_ops, "dense_reduce_by_key", spy)
    dk = (torch.randperm(20_000)[:12_000] * 4 + 1).cuda()                          # owner 1 of p = 4
    dv = torch.randn(12_000, 16, device="cuda")
    plan = sparse._dense_plan(sparse.KeyRange(int(dk.min()), int(dk.max()), None), 4, dk)
    assert plan is not None
    uk, uv, _ = sparse._reduce_by_key(dk, dv, op, None, plan)
    rk, rv, _ = device_ops.reduce_by_key(dk, dv, 0)
    assert calls == [True] and torch.equal(uk, rk) and torch.equal(uv, rv)


def _table_fn(comm):
    import numpy as np
    from mp4x import Operators
    from mp4x.ops import device_ops
    r = comm.getRank()
    used = {"dense": 0, "canonical": 0}
    real_d, real_c = device_ops.dense_reduce_by_key, device_ops.hash_reduce_by_key_canonical

    def spy_d(*a, **k):
        out = real_d(*a, **k)
        used["dense"] += out is not None
        return out

    def spy_c(*a, **k):
        used["canonical"] += 1
        return real_c(*a, **k)
    device_ops.dense_reduce_by_key, device_ops.hash_reduce_by_key_canonical = spy_d, spy_c
    g = torch.Generator().manual_seed(70 + r)
    pool = torch.randint(-(1 << 62), 1 << 62, (9000,), generator=torch.Generator().manual_seed(1))   # sparse 64-bit ids
    keys = pool[torch.randperm(9000, generator=g)[:6000]].unique().cuda()           # overlapping between the ranks
    vals = torch.randint(-8, 8, (keys.numel(), 16), generator=g).float().cuda()
    ak, av = comm.allreduceSparse(keys, vals, Operators.Float.SUM)
    assert used == {"dense": 0, "canonical": 0}
    t1 = comm.allreduceSparse(keys, vals, Operators.Float.SUM, keyOrder="table")
    t2 = comm.allreduceSparse(keys, vals, Operators.Float.SUM, keyOrder="table")
    sparse_used = dict(used)
    dkeys = torch.randperm(30_000, generator=g)[:20_000].cuda()                      # dense ids: K5d
    dvals = torch.randint(-8, 8, (20_000, 16), generator=g).float().cuda()
    da = comm.allreduceSparse(dkeys, dvals, Operators.Float.SUM)
    dt = comm.allreduceSparse(dkeys, dvals, Operators.Float.SUM, keyOrder="table")
    torch.cuda.synchronize()
    same_calls = torch.equal(t1[0], t2[0]) and torch.equal(t1[1], t2[1])
    dense_same = torch.equal(da[0], dt[0]) and torch.equal(da[1], dt[1])
    n = lambda x: x.cpu().numpy()   # noqa: E731 — numpy crosses the result queue, tensors do not
    return n(ak), n(av), n(t1[0]), n(t1[1]), same_calls, sparse_used, dict(used), dense_same, np.int64(r)


def test_allreduce_sparse_with_key_order_table_on_two_ranks():
    out = run_spawn(2, _table_fn)
    import numpy as np
    (ak0, av0, tk0, tv0, same0, su0, u0, ds0, _), (ak1, av1, tk1, tv1, same1, su1, u1, ds1, _) = out[0], out[1]
    assert same0 and same1                                    # two calls: the same tensors
    assert np.array_equal(tk0, tk1) and np.array_equal(tv0, tv1)          # both ranks: the same tensors
    o_a, o_t = np.argsort(ak0), np.argsort(tk0)
    assert np.array_equal(ak0[o_a], tk0[o_t]) and np.array_equal(av0[o_a], tv0[o_t])   # the pairs of "ascending"
    assert not np.array_equal(ak0, tk0)                       # in another order
    for su, u, ds in ((su0, u0, ds0), (su1, u1, ds1)):
        assert su == {"dense": 0, "canonical": 2}             # sparse ids: K5c, once per call
        assert u == {"dense": 2, "canonical": 2} and ds       # dense ids: K5d whatever the key order
