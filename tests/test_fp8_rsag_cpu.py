"""The host side of the fp8 reduce-scatter / all-gather, without a GPU: every refusal of the two
``_check`` entry points on the real libmp4x_hip.so (fake pointers: the checks are host-side and
launch nothing), and ZeroOptimizer(grad_codec=...) on the CPU / gloo path, where there is no mesh
and the gradients therefore take the exact reduce-scatter."""
import ctypes

import pytest

torch = pytest.importorskip("torch")

from harness import run_ranks  # noqa: E402
from mp4x.operators import DType  # noqa: E402
from mp4x.ops import native  # noqa: E402

BADARG, UNSUPPORTED = 1001, 1002
I64 = ctypes.c_int64


def _lib():
    try:
        import mp4x.parallel.ipc  # noqa: F401  (registers the ipc signatures)
        return native.hip()
    except Exception as e:   # noqa: BLE001
        pytest.skip(f"libmp4x_hip.so not loadable: {e}")


def _check(lib, half, dtype=DType.F32, rank=0, p=2, nblk=4, soff=1024, lo=(0, 260), hi=(260, 768), out=0x1000):
    fn = lib.mp4x_ipc_fp8_reduce_scatter_check if half == "rs" else lib.mp4x_ipc_fp8_allgather_check
    n = max(len(lo), 1)
    return fn(int(dtype), rank, p, nblk, soff, (I64 * n)(*lo), (I64 * n)(*hi), out)


@pytest.mark.parametrize("half", ["rs", "ag"])
def test_check_accepts_a_valid_call(half):
    lib = _lib()
    assert _check(lib, half) == 0
    assert _check(lib, half, dtype=DType.BF16, rank=2, p=3, lo=(0, 260, 260), hi=(260, 260, 768)) == 0   # an empty segment
    assert _check(lib, half, dtype=DType.F16, rank=7, p=8, lo=(0,) * 8, hi=(4,) * 8 if half == "ag" else (0,) * 7 + (4,)) == 0


@pytest.mark.parametrize("half", ["rs", "ag"])
@pytest.mark.parametrize("case,want", [
    (dict(dtype=DType.F64), UNSUPPORTED),                       # dtype not f32 / bf16 / f16
    (dict(dtype=DType.I32), UNSUPPORTED),
    (dict(p=1, lo=(0,), hi=(4,)), BADARG),                      # p outside 2..8
    (dict(p=9, lo=(0,) * 9, hi=(0,) * 9), BADARG),
    (dict(rank=-1), BADARG),                                    # rank outside [0, p)
    (dict(rank=2), BADARG),
    (dict(lo=(0, 260), hi=(260, 256)), BADARG),                 # a descending segment
    (dict(lo=(0, 260), hi=(260, 1288)), BADARG),                # past the 4 quantised blocks (either half's rule)
    (dict(out=0x1008), BADARG),                                 # out not 16-byte aligned
    (dict(soff=1028), BADARG),                                  # soff not 16-byte aligned
    (dict(soff=1008), BADARG),                                  # scales inside the q bytes
])
def test_check_refuses_without_launching(half, case, want):
    assert _check(_lib(), half, **case) == want


def test_reduce_scatter_check_wants_ascending_segments():
    """The reduce-scatter's segments tile one range in rank order; the all-gather's may land anywhere."""
    lib = _lib()
    assert _check(lib, "rs", lo=(260, 0), hi=(768, 260)) == BADARG
    assert _check(lib, "ag", nblk=4, lo=(260, 0), hi=(768, 260)) == 0


# ---------------------------------------------------------------- ZeroOptimizer(grad_codec=...)
def _zero(comm, codec):
    from mp4x.models.zero import train_zero
    return train_zero(comm, steps=6, global_batch=48, grad_codec=codec)


def test_zero_grad_codec_is_exact_without_a_mesh():
    plain, _, _ = run_ranks(2, _zero, (None,), timeout=120)
    coded, _, _ = run_ranks(2, _zero, ("fp8",), timeout=120)
    assert sorted(plain) == sorted(coded) == [0, 1]
    for r in plain:
        assert coded[r] == plain[r]                             # the loss list, exactly


class _Solo:
    def getSlaveNum(self):
        return 1

    def getRank(self):
        return 0


def test_zero_grad_codec_operands():
    from mp4x.models.zero import ZeroOptimizer
    a = torch.nn.Linear(6, 3)
    z = ZeroOptimizer(_Solo(), a.parameters(), torch.optim.SGD, lr=0.1)
    assert z.grad_codec is None
    for b in z.buckets:
        assert b.grad_operand is b.operand and b.operand.codec is None     # the single operand
    z = ZeroOptimizer(_Solo(), torch.nn.Linear(6, 3).parameters(), torch.optim.SGD, lr=0.1, grad_codec="fp8")
    for b in z.buckets:
        assert b.grad_operand is not b.operand
        assert b.grad_operand.codec == "fp8" and b.operand.codec is None   # the parameter all-gather stays exact
        assert b.grad_operand.dtype == b.operand.dtype


def test_zero_grad_codec_refuses_f64_and_unknown_codecs():
    from mp4x.models.zero import ZeroOptimizer
    with pytest.raises(ValueError):
        ZeroOptimizer(_Solo(), torch.nn.Linear(6, 3).double().parameters(), torch.optim.SGD, lr=0.1, grad_codec="fp8")
    with pytest.raises(ValueError):
        ZeroOptimizer(_Solo(), torch.nn.Linear(6, 3).parameters(), torch.optim.SGD, lr=0.1, grad_codec="zlib")
    ZeroOptimizer(_Solo(), torch.nn.Linear(6, 3).double().parameters(), torch.optim.SGD, lr=0.1)   # f64 alone is fine
