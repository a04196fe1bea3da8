"""The (dtype, op) table of the native library, swept from outside: which pairs the IPC tier and
the hash reduce-by-key serve, that the Python-side ``ipc_op_ok`` agrees, and the refusal code of
every entry point that turns a runtime (dtype, op) into a kernel.  CPU: the real libmp4x_hip.so,
called with dummy pointers and INVALID pairs only (a refusal returns before any launch; a valid
pair would launch)."""
import ctypes
import types

import pytest

torch = pytest.importorskip("torch")

from mp4x.operators import DType, OpCode, dtype_of_torch  # noqa: E402
from mp4x.ops import native  # noqa: E402

BADARG, UNSUPPORTED = 1001, 1002
DTYPES = range(-1, 10)           # 0..8 are the dtypes of the table
OPS = range(-1, 13)              # 0..10 the operator table, 11 the FIRST rule
FIRST = 11
FLOATS = {DType.F64, DType.F32, DType.BF16, DType.F16}
INTS = {DType.I64, DType.I32, DType.I16, DType.I8, DType.U8}


def _lib():
    try:
        import mp4x.parallel.ipc  # noqa: F401  (registers the ipc signatures)
        return native.hip()
    except Exception as e:   # noqa: BLE001
        pytest.skip(f"libmp4x_hip.so not loadable: {e}")


def _table_ok(dt, op):
    """The operator table, written out: SUM / MAX / MIN / PROD for all 9 dtypes, BAND / BOR / BXOR
    for the 5 integer dtypes, F*LOC for f64 only, I*LOC for i64 only."""
    if dt not in FLOATS | INTS:
        return False
    if op in (OpCode.SUM, OpCode.MAX, OpCode.MIN, OpCode.PROD):
        return True
    if op in (OpCode.BAND, OpCode.BOR, OpCode.BXOR):
        return dt in INTS
    if op in (OpCode.FMAXLOC, OpCode.FMINLOC):
        return dt == DType.F64
    if op in (OpCode.IMAXLOC, OpCode.IMINLOC):
        return dt == DType.I64
    return False                  # FIRST, and everything outside 0..11


def _row_ok(dt, op):
    """The hash / dense reduce-by-key: the table without the LOC ops (and without FIRST)."""
    return _table_ok(dt, op) and op <= OpCode.BXOR


def test_ipc_op_supported_is_the_operator_table():
    lib = _lib()
    got = {(dt, op): lib.mp4x_ipc_op_supported(dt, op) for dt in DTYPES for op in OPS}
    assert got == {(dt, op): int(_table_ok(dt, op)) for dt in DTYPES for op in OPS}
    assert sum(got.values()) == 9 * 4 + 5 * 3 + 2 + 2


def test_hash_rbk_supported_is_the_table_without_loc_and_first():
    lib = _lib()
    got = {(dt, op): lib.mp4x_hash_rbk_supported(dt, op) for dt in DTYPES for op in OPS}
    assert got == {(dt, op): int(_row_ok(dt, op)) for dt in DTYPES for op in OPS}
    assert sum(got.values()) == 9 * 4 + 5 * 3


def test_python_ipc_op_ok_agrees_with_the_native_table():
    from mp4x.parallel.ipc import SUPPORTED_DTYPES, ipc_op_ok
    lib = _lib()
    assert len(SUPPORTED_DTYPES) == 9
    for tdt in SUPPORTED_DTYPES:
        for code in OpCode:
            op = types.SimpleNamespace(code=code, is_custom=False)
            assert ipc_op_ok(tdt, op) == bool(lib.mp4x_ipc_op_supported(int(dtype_of_torch(tdt)), int(code))), \
                (tdt, code)


# dummy non-null, 16-byte-aligned pointers: never dereferenced by a call that is refused
P = [0x10000 * (k + 1) for k in range(8)]


def test_reduce_refusal_codes():
    lib = _lib()
    ins, _keep = native.ptr_array([P[1], P[2]])
    for dt in DTYPES:
        for op in OPS:
            if _table_ok(dt, op):
                continue                                  # a valid pair would launch
            rc = lib.mp4x_reduce(dt, op, P[0], ins, 2, 1, None)
            if not 0 <= dt <= 8:
                want = BADARG                             # unknown dtype, whatever the op
            elif not 0 <= op <= 10:
                want = BADARG                             # not an operator of K1 (FIRST included)
            else:
                want = UNSUPPORTED                        # in range, but not a pair of the table
            assert rc == want, (dt, op)
    # unknown dtype with an op that is valid elsewhere
    assert lib.mp4x_reduce(9, int(OpCode.SUM), P[0], ins, 2, 1, None) == BADARG
    assert lib.mp4x_reduce(-1, int(OpCode.SUM), P[0], ins, 2, 1, None) == BADARG


def test_segment_reduce_refusal_codes():
    lib = _lib()
    for dt in DTYPES:
        for op in OPS:
            if _row_ok(dt, op) or (0 <= dt <= 8 and op == FIRST):
                continue                                  # the segmented reduce serves FIRST too
            rc = lib.mp4x_segment_reduce_rows(dt, op, P[0], P[1], P[2], P[3], 1, 1, P[4], 1, P[5], P[6], P[7], None)
            assert rc == UNSUPPORTED, (dt, op)


def test_hash_and_dense_reduce_by_key_refusal_codes():
    lib = _lib()
    for dt in DTYPES:
        for op in OPS:
            if lib.mp4x_hash_rbk_supported(dt, op):
                continue
            rc = lib.mp4x_hash_reduce_by_key(dt, op, P[0], 1, P[1], 1, P[2], 1 << 20, P[3], P[4], P[5], P[6], None)
            assert rc == UNSUPPORTED, (dt, op)
            rc = lib.mp4x_dense_reduce_by_key(dt, op, P[0], 1, P[1], 1, 0, 1, 64, P[2], 1 << 20, P[3], P[4], P[5],
                                              P[6], None)
            assert rc == UNSUPPORTED, (dt, op)


def test_scale_refusal_codes():
    lib = _lib()
    for dt in DTYPES:
        if dt in FLOATS:
            continue
        assert lib.mp4x_scale(dt, P[0], P[1], 0.5, 1, None) == UNSUPPORTED, dt
