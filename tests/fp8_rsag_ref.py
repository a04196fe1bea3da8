"""The contract of the fp8 reduce-scatter / all-gather (reduceScatterArray / allgatherArray with the
fp8 operand), computed with the CPU reference of the K6 codec (tests/fp8_ref.py), and the cases
the GPU tests run.  Shared by tests/test_ipc_fp8_rsag_gpu.py and tests/test_fp8_rsag_api_gpu.py.

With Q = ref_quant, R = ref_dequant_reduce, S = ref_store:

* reduce-scatter: on rank r, x[f_r:t_r] is the slice [f_r - base, t_r - base) of
  S(R([Q(x_0[base:end]), ..., Q(x_{p-1}[base:end])])); every other element keeps its input bits;
* all-gather: on every rank, x[f_k:t_k] is S(R([Q(x_k[f_k:t_k])])) for every k, the rank's own
  segment included; elements outside the range keep their input bits.
"""
import torch

from fp8_ref import ref_dequant_reduce, ref_quant, ref_store

# case -> (dtype name, tensor n, frm, {p: counts})
CASES = {
    "A": ("float32", 768, 0, {2: [260, 508], 3: [260, 0, 508]}),          # a block shared by two ranks; an empty segment
    "B": ("float32", 1200, 8, {2: [300, 100], 3: [300, 96, 4]}),          # a range inside a larger tensor, partial last block
    "C": ("float32", 200_000, 0, {2: [100_000, 100_000], 3: [66_668, 66_664, 66_668]}),   # several pieces
    "D": ("bfloat16", 70_000, 0, {2: [35_000, 35_000], 3: [23_336, 23_328, 23_336]}),     # 16-bit store; pieces
    "E": ("float16", 2064, 0, {2: [1032, 1032], 3: [1024, 8, 1032]}),     # f16; a segment smaller than a block
}


def inputs(n, dtype, p):
    """Every rank's input, built on the CPU, the same in every process."""
    return [torch.randn(n, generator=torch.Generator().manual_seed(500 + j)).to(dtype) for j in range(p)]


def bounds(frm, counts):
    froms, tos, o = [], [], frm
    for c in counts:
        froms.append(o)
        o += c
        tos.append(o)
    return froms, tos


def bits(t):
    """The tensor's bits as integers (a comparison that tells -0 from +0 and equal NaNs as equal)."""
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def same_bits(a, b):
    return bool(torch.equal(bits(a), bits(b)))


def expect_reduce_scatter(xs, r, frm, counts):
    """(rank r's whole tensor after the call, ambiguous)."""
    froms, tos = bounds(frm, counts)
    base, end = froms[0], tos[-1]
    qs, ss = zip(*[ref_quant(x[base:end]) for x in xs])
    acc, amb = ref_dequant_reduce(list(qs), list(ss))
    full = ref_store(acc, xs[0].dtype)
    out = xs[r].clone()
    out[froms[r]:tos[r]] = full[froms[r] - base:tos[r] - base]
    return out, amb


def expect_allgather(xs, r, frm, counts):
    """(rank r's whole tensor after the call, ambiguous)."""
    froms, tos = bounds(frm, counts)
    out = xs[r].clone()
    amb = 0
    for k, (f, t) in enumerate(zip(froms, tos)):
        if t == f:
            continue
        q, s = ref_quant(xs[k][f:t])
        acc, a = ref_dequant_reduce([q], [s])
        amb += a
        out[f:t] = ref_store(acc, xs[0].dtype)[:t - f]
    return out, amb
