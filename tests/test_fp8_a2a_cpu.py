"""The host side of the fp8 ragged all-to-all, without a GPU: the geometry (IpcAllreduce.fp8_a2a_plan,
a pure function), the contract helper against a direct per-row slice, every refusal of
``mp4x_ipc_fp8_alltoall_check`` on the real libmp4x_hip.so (fake pointers: the check is host-side and
launches nothing), and alltoallArray with the fp8 operand on the CPU / gloo path, where there is no
mesh and the call is therefore the exact one."""
import ctypes
import random

import pytest

torch = pytest.importorskip("torch")

from fp8_a2a_ref import CASES, TOO_LARGE, exact_alltoall, expect_alltoall, inputs, same_bits  # noqa: E402
from fp8_ref import ref_dequant_reduce, ref_quant, ref_store  # noqa: E402
from harness import run_ranks  # noqa: E402
from mp4x.operators import DType  # noqa: E402
from mp4x.ops import native  # noqa: E402

BADARG, UNSUPPORTED = 1001, 1002
I64 = ctypes.c_int64
Q = 256


# ---------------------------------------------------------------- the geometry
def _check_plans(mat, w, cap):
    from mp4x.parallel.ipc import IpcAllreduce
    p = len(mat)
    largest = max(-(-sum(row) * w // Q) for row in mat)
    plans = [IpcAllreduce.fp8_a2a_plan(mat, w, r, cap) for r in range(p)]
    if largest > cap:
        assert plans == [None] * p                            # exactly when the largest send does not fit
        return None
    assert None not in plans
    for r, pl in enumerate(plans):
        off = 0
        for k in range(p):
            assert pl.elo[k] == sum(mat[k][:r]) * w
            assert pl.ehi[k] - pl.elo[k] == mat[k][r] * w
            assert pl.dst[k] == off                           # rank order, no gap, no overlap
            off += pl.ehi[k] - pl.elo[k]
            assert pl.nblk_peer[k] == -(-sum(mat[k]) * w // Q)
            assert pl.ehi[k] <= pl.nblk_peer[k] * Q
        assert off == sum(mat[k][r] for k in range(p)) * w    # ... and the ranges tile the receive tensor
        assert pl.soff == plans[0].soff and pl.steps == plans[0].steps
        assert pl.soff % 16 == 0 and pl.soff >= largest * Q
    # the grid covers the largest (sender, receiver) segment anywhere in the matrix
    seg = 0
    for k in range(p):
        for j in range(p):
            lo, hi = sum(mat[k][:j]) * w, sum(mat[k][:j + 1]) * w
            if hi > lo:
                seg = max(seg, -(-hi // Q) - lo // Q)
    assert plans[0].steps == -(-seg // 4)
    return plans


def test_plan_on_the_cases():
    for _, w, mats in list(CASES.values()):
        for mat in mats.values():
            assert _check_plans(mat, w, 252) is not None
    for mat in TOO_LARGE[2].values():
        assert _check_plans(mat, TOO_LARGE[1], 252) is None   # 275 blocks against 252
        assert _check_plans(mat, TOO_LARGE[1], 275) is not None


def test_plan_on_random_matrices():
    rng = random.Random(20240612)
    fit = 0
    for _ in range(200):
        p = rng.randint(2, 8)
        w = rng.choice([4, 8, 12, 64, 256])
        top = rng.choice([0, 1, 3, 40, 400])
        mat = [[rng.randint(0, top) if rng.random() < 0.8 else 0 for _ in range(p)] for _ in range(p)]
        cap = rng.choice([1, 8, 252, 1 << 20])
        fit += _check_plans(mat, w, cap) is not None
    assert 20 < fit < 200                                      # both outcomes were drawn


def test_plan_refuses_a_width_off_the_4_element_grid():
    from mp4x import Mp4jException
    from mp4x.parallel.ipc import IpcAllreduce
    with pytest.raises(Mp4jException):
        IpcAllreduce.fp8_a2a_plan([[1, 1], [1, 1]], 3, 0, 252)


def test_grid_cap_family_resolves_from_the_resource_table():
    """Family ``fp8a2a`` = ``k_ipc_fp8_a2a<DT, NR>`` in the build's resource table, every
    instantiation, and no fewer resident blocks than the all-gather it is modelled on."""
    import os
    from mp4x.parallel import occupancy as occ
    from mp4x.parallel.ipc import IpcAllreduce
    assert IpcAllreduce._OCC_FAMILY["fp8a2a"] == 6
    assert occ._FAMILY_KERNEL["fp8a2a"] == "k_ipc_fp8_a2a"
    if not os.path.exists(occ._table_path()):
        pytest.skip("native library not built")
    for dt in (DType.F32, DType.BF16, DType.F16):
        for p in range(2, 9):
            bpc = occ.table_bpc("fp8a2a", int(dt), dt.name, 0, p)
            assert bpc is not None and bpc >= 1, (dt, p)
            assert bpc >= occ.table_bpc("fp8ag", int(dt), dt.name, 0, p), (dt, p)


# ---------------------------------------------------------------- the contract helper
def test_contract_equals_a_per_row_slice():
    """Case D (rows of 12 straddle the 256-element blocks): every received row is the sender's row
    of S(R([Q(flat)])), looked up one row at a time."""
    dtype_name, w, mats = CASES["D"]
    dt = getattr(torch, dtype_name)
    for p, mat in mats.items():
        sends = inputs(mat, w, dt)
        full = []
        for s in sends:
            q, sc = ref_quant(s.reshape(-1))
            acc, amb = ref_dequant_reduce([q], [sc])
            assert amb == 0
            full.append(ref_store(acc, dt))
        for r in range(p):
            want, counts, amb = expect_alltoall(sends, mat, w, r)
            assert amb == 0 and counts == [mat[k][r] for k in range(p)]
            assert tuple(want.shape) == (sum(counts), w)
            row = 0
            for k in range(p):
                for i in range(mat[k][r]):
                    src = sum(mat[k][:r]) + i
                    assert same_bits(want[row], full[k][src * w:(src + 1) * w]), (p, r, k, i)
                    row += 1
            # e4m3 on the wire: close to the senders' rows, and not equal to them
            exact = exact_alltoall(sends, mat, r)
            assert not torch.equal(want, exact)
            assert float((want - exact).abs().max()) <= float(exact.abs().max()) / 16


# ---------------------------------------------------------------- the native check
def _lib():
    try:
        import mp4x.parallel.ipc  # noqa: F401  (registers the ipc signatures)
        return native.hip()
    except Exception as e:   # noqa: BLE001
        pytest.skip(f"libmp4x_hip.so not loadable: {e}")


def _case_a(rank=1, p=2):
    from mp4x.parallel.ipc import IpcAllreduce
    _, w, mats = CASES["A"]
    return IpcAllreduce.fp8_a2a_plan(mats[p], w, rank, 252)


def _check(lib, dtype=DType.F32, rank=1, p=2, out=0x1000, **over):
    pl = _case_a(rank if 0 <= rank < p else 0, p if p in (2, 3) else 2)._asdict()
    pl.update(over)
    n = max(p, 1, len(pl["elo"]))

    def arr(v):
        v = list(v) + [0] * (n - len(v))
        return (I64 * n)(*v)
    return lib.mp4x_ipc_fp8_alltoall_check(int(dtype), rank, p, pl["soff"], arr(pl["elo"]), arr(pl["ehi"]),
                                           arr(pl["dst"]), arr(pl["nblk_peer"]), out)


def test_check_accepts_case_a():
    lib = _lib()
    for p in (2, 3):
        for r in range(p):
            assert _check(lib, rank=r, p=p) == 0
    assert _check(lib, dtype=DType.BF16) == 0
    assert _check(lib, dtype=DType.F16) == 0
    # a rank that receives nothing may have no tensor to point to
    assert _check(lib, elo=[0, 0], ehi=[0, 0], dst=[0, 0], out=0) == 0


# case A, p = 2, rank 1: elo = [260, 0], ehi = [380, 516], dst = [0, 120], nblk_peer = [2, 3], soff = 768
@pytest.mark.parametrize("case,want", [
    (dict(dtype=DType.F64), UNSUPPORTED),                       # dtype not f32 / bf16 / f16
    (dict(dtype=DType.I32), UNSUPPORTED),
    (dict(p=1), BADARG),                                        # p outside 2..8
    (dict(p=9), BADARG),
    (dict(rank=-1), BADARG),                                    # rank outside [0, p)
    (dict(rank=2), BADARG),
    (dict(elo=[-4, 0]), BADARG),                                # a negative offset
    (dict(elo=[384, 0]), BADARG),                               # a descending range
    (dict(elo=[262, 0]), BADARG),                               # offsets off the 4-element grid
    (dict(ehi=[382, 516]), BADARG),
    (dict(dst=[0, 122]), BADARG),                               # ... which also breaks dst - elo
    (dict(ehi=[516, 516], dst=[0, 256]), BADARG),               # past peer 0's 2 quantised blocks
    (dict(nblk_peer=[2, 2]), BADARG),                           # peer 1's range past its blocks
    (dict(nblk_peer=[2, -1]), BADARG),
    (dict(soff=512), BADARG),                                   # scales inside the q bytes
    (dict(soff=776), BADARG),                                   # soff not 16-byte aligned
    (dict(out=0x1008), BADARG),                                 # out not 16-byte aligned
    (dict(out=0), BADARG),                                      # rows to receive and nowhere to put them
    (dict(dst=[0, 116]), BADARG),                               # overlapping ranges in the receive tensor
])
def test_check_refuses_without_launching(case, want):
    assert _check(_lib(), **case) == want


def test_case_a_geometry_is_what_the_refusals_assume():
    pl = _case_a()
    assert (pl.elo, pl.ehi, pl.dst, pl.nblk_peer, pl.soff) == ([260, 0], [380, 516], [0, 120], [2, 3], 768)


# ---------------------------------------------------------------- the public API without a mesh
def _gloo_a2a(comm):
    from mp4x import Operands
    r, p = comm.getRank(), comm.getSlaveNum()
    _, w, mats = CASES["A"]
    mat = mats[p]
    sends = inputs(mat, w, torch.float32)
    plain, rc0 = comm.alltoallArray(sends[r].clone(), mat[r])
    before = dict(comm.device.stats)
    coded, rc1 = comm.alltoallArray(sends[r].clone(), mat[r], operand=Operands.FLOAT_OPERAND(codec="fp8"))
    used = {k: c - before.get(k, 0) for k, c in comm.device.stats.items() if c != before.get(k, 0)}
    given = torch.empty_like(coded)
    got, rc2 = comm.alltoall_array(sends[r].clone(), mat[r], given, Operands.FLOAT_OPERAND(codec="fp8"))
    want = exact_alltoall(sends, mat, r)
    return dict(exact=same_bits(plain, want) and same_bits(coded, want) and same_bits(given, want),
                same=got is given, counts=(rc0, rc1, rc2), want_counts=[mat[k][r] for k in range(p)], used=used)


@pytest.mark.parametrize("p", [2, 3])
def test_fp8_operand_on_host_tensors_is_the_exact_call(p):
    res, _, _ = run_ranks(p, _gloo_a2a, timeout=120)
    assert sorted(res) == list(range(p))
    for r, row in res.items():
        assert row["exact"], r
        assert row["same"], r
        assert row["counts"] == (row["want_counts"],) * 3, (r, row["counts"])
        assert row["used"] == {"all_to_all_v": 1}, (r, row["used"])    # no fp8 counter
