"""The contract of the fp8 ragged all-to-all (alltoallArray with the fp8 operand), computed with the
CPU reference of the K6 codec (tests/fp8_ref.py), and the cases the tests run.  Shared by
tests/test_ipc_fp8_a2a_gpu.py, tests/test_fp8_a2a_api_gpu.py and tests/test_fp8_a2a_cpu.py.

With Q = ref_quant, R = ref_dequant_reduce, S = ref_store, w the row width in elements and
mat[k][j] the rows rank k sends to rank j: rank k's send buffer, flattened, is quantised on ONE
256-element block grid counted from its first element, and on rank r

    recv = concat over k of S(R([Q(send_k.flatten())]))[lo_k * w : (lo_k + mat[k][r]) * w],
    lo_k = sum(mat[k][:r]),

the rows in source-rank order.  recvCounts[k] = mat[k][r], as in the exact call.
"""
import torch

from fp8_ref import ref_dequant_reduce, ref_quant, ref_store
from fp8_rsag_ref import bits, same_bits  # noqa: F401  (re-exported for the tests)

# case -> (dtype name, row width, {p: mat})
CASES = {
    # a block shared by two destinations; an empty segment; a partial last block; a rank that sends nothing
    "A": ("float32", 4, {2: [[65, 30], [0, 129]], 3: [[65, 0, 30], [0, 129, 1], [0, 0, 0]]}),
    # 16-bit store; one-row segments
    "B": ("bfloat16", 8, {2: [[33, 31], [70, 5]], 3: [[33, 31, 3], [70, 5, 64], [1, 1, 1]]}),
    # rows equal to blocks
    "C": ("float16", 256, {2: [[2, 1], [0, 3]], 3: [[2, 1, 1], [0, 3, 0], [1, 0, 2]]}),
    # rows that straddle blocks
    "D": ("float32", 12, {2: [[100, 57], [43, 200]], 3: [[100, 57, 9], [43, 200, 0], [7, 0, 150]]}),
    # 128 blocks: several kernel blocks and wave steps; 33,296 bytes of a 64 KiB buffer
    "E": ("float32", 64, {2: [[300, 212], [180, 256]], 3: [[300, 100, 112], [180, 200, 56], [0, 330, 150]]}),
}

# does not fit a 64 KiB buffer: rank 0 sends 1100 rows of 64 f32 = 275 quant blocks against 252
TOO_LARGE = ("float32", 64, {2: [[600, 500], [3, 2]], 3: [[600, 300, 200], [3, 2, 1], [0, 1, 0]]})


def inputs(mat, w, dtype):
    """Every rank's send tensor [rows_i, w], built on the CPU, the same in every process."""
    return [torch.randn(sum(row), w, generator=torch.Generator().manual_seed(700 + i)).to(dtype)
            for i, row in enumerate(mat)]


def decoded(send, dtype):
    """(S(R([Q(send.flatten())])) cut to the send's elements, ambiguous): what any receiver decodes."""
    n = send.numel()
    if n == 0:
        return torch.empty(0, dtype=dtype), 0
    q, s = ref_quant(send.reshape(-1))
    acc, amb = ref_dequant_reduce([q], [s])
    return ref_store(acc, dtype)[:n], amb


def expect_alltoall(sends, mat, w, r):
    """(rank r's receive tensor [rows, w], recvCounts, ambiguous)."""
    dtype = sends[0].dtype
    parts, amb = [], 0
    for k, send in enumerate(sends):
        full, a = decoded(send, dtype)
        amb += a
        lo = sum(mat[k][:r])
        parts.append(full[lo * w:(lo + mat[k][r]) * w])
    counts = [mat[k][r] for k in range(len(mat))]
    return torch.cat(parts).view(sum(counts), w), counts, amb


def exact_alltoall(sends, mat, r):
    """Rank r's receive tensor of the exact call: the senders' rows, bit for bit."""
    return torch.cat([sends[k][sum(mat[k][:r]):sum(mat[k][:r + 1])] for k in range(len(mat))])
