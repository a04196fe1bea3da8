"""torch-facing wrappers of the native CDNA4 kernels.

Every wrapper validates shapes, dtypes, devices and contiguity on the host BEFORE the
launch (a bad pointer on a GPU is a machine-wide fault, not an exception) and launches on
the current torch stream.
"""
from __future__ import annotations

import os
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from ..operators import DType, dtype_of_torch
from . import native
from .native import check, ptr_array, stream_ptr

QBLOCK = 256
MAX_NIN = 8      # MP4X_MAX_NIN (csrc/include/mp4x/ops.h): inputs per launch, chained beyond


def _dev_check(*ts):
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise ValueError("device op needs GPU tensors")
        if not t.is_contiguous():
            raise ValueError("device op needs contiguous tensors")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise ValueError("all tensors must be on one device")


def reduce_(out: torch.Tensor, inputs: Sequence[torch.Tensor], op: int, dtype: Optional[DType] = None,
            stream=None) -> torch.Tensor:
    """out = op(inputs[0], inputs[1], ...) elementwise, in input order (out may alias inputs[0])."""
    if not inputs:
        raise ValueError("no inputs")
    _dev_check(out, *inputs)
    n = out.numel()
    for t in inputs:
        if t.numel() != n or t.dtype != out.dtype:
            raise ValueError(f"reduce_: shape/dtype mismatch {t.shape}/{t.dtype} vs {out.shape}/{out.dtype}")
    dt = dtype if dtype is not None else dtype_of_torch(out.dtype)
    pp, keep = ptr_array([t.data_ptr() for t in inputs])
    check(native.hip().mp4x_reduce(int(dt), int(op), out.data_ptr(), pp, len(inputs), n, stream_ptr(stream)),
          "mp4x_reduce")
    return out


def reduce_strided_(out: torch.Tensor, base: torch.Tensor, nin: int, op: int, stream=None) -> torch.Tensor:
    """out = op over nin equal chunks of ``base`` (laid out back to back, each out.numel() long)."""
    _dev_check(out, base)
    n = out.numel()
    if base.numel() < n * nin or base.dtype != out.dtype:
        raise ValueError("reduce_strided_: base too small or dtype mismatch")
    dt = dtype_of_torch(out.dtype)
    check(native.hip().mp4x_reduce_strided(int(dt), int(op), out.data_ptr(), base.data_ptr(), n, nin, n,
                                           stream_ptr(stream)), "mp4x_reduce_strided")
    return out


def scale_(out: torch.Tensor, inp: torch.Tensor, s: float, stream=None) -> torch.Tensor:
    _dev_check(out, inp)
    if out.numel() != inp.numel() or out.dtype != inp.dtype:
        raise ValueError("scale_: mismatch")
    check(native.hip().mp4x_scale(int(dtype_of_torch(out.dtype)), out.data_ptr(), inp.data_ptr(), float(s),
                                  out.numel(), stream_ptr(stream)), "mp4x_scale")
    return out


def segment_copy_(dst: torch.Tensor, src: torch.Tensor, segs: Sequence[Tuple[int, int, int]], stream=None):
    """segs = [(dst_elem_off, src_elem_off, nelems)] copied in one launch."""
    _dev_check(dst, src)
    if not segs:
        return dst
    es = dst.element_size()
    if src.element_size() != es:
        raise ValueError("segment_copy_: element size mismatch")
    dn, sn = dst.numel(), src.numel()
    for d, s, l in segs:
        if d < 0 or s < 0 or l < 0 or d + l > dn or s + l > sn:
            raise ValueError(f"segment_copy_: segment {(d, s, l)} out of bounds ({dn}, {sn})")
    segs = [x for x in segs if x[2] > 0]
    if not segs:
        return dst
    table = torch.tensor([d * es for d, _, _ in segs] + [s * es for _, s, _ in segs] + [l * es for _, _, l in segs],
                         dtype=torch.int64).pin_memory().to(dst.device, non_blocking=True)
    max_len = max(l for _, _, l in segs) * es
    check(native.hip().mp4x_segment_copy(dst.data_ptr(), src.data_ptr(), table.data_ptr(), len(segs), max_len,
                                         stream_ptr(stream)), "mp4x_segment_copy")
    # `table` may be freed right away: the caching allocator only reuses it in stream order
    return dst


def gather_rows(inp: torch.Tensor, idx: torch.Tensor, out: Optional[torch.Tensor] = None, stream=None):
    """out[i] = inp[idx[i]] for a 2-D (rows, ...) tensor."""
    _dev_check(inp, idx)
    if idx.dtype != torch.int64:
        raise ValueError("gather_rows: idx must be int64")
    rows = inp.shape[0]
    row_bytes = inp[0].numel() * inp.element_size() if rows else 0
    if out is None:
        out = torch.empty((idx.numel(),) + tuple(inp.shape[1:]), dtype=inp.dtype, device=inp.device)
    _dev_check(out)
    check(native.hip().mp4x_gather_rows(out.data_ptr(), inp.data_ptr(), idx.data_ptr(), idx.numel(), row_bytes,
                                        stream_ptr(stream)), "mp4x_gather_rows")
    return out


# ------------------------------------------------------------------ fp8 codec (K6)
# The buffer contract of the codec is WHOLE BLOCKS: the kernels move one dword per lane for every
# lane of the last block, so a code buffer for n elements is nblk * 256 bytes (nblk = ceil(n / 256)),
# and the quantiser writes the pad past n as zero codes.  The re-quantising dequant-reduce folds
# the pad lanes into the last block's amax, so its inputs must carry that zero pad.
def _room(t: torch.Tensor) -> int:
    """Bytes from t's first element to the end of the allocation it is a view of."""
    return t.untyped_storage().nbytes() - t.storage_offset() * t.element_size()


def quant_fp8(x: torch.Tensor, q: Optional[torch.Tensor] = None, scales: Optional[torch.Tensor] = None,
              stream=None):
    """Block-scaled e4m3 quantisation (256 elements / scale). Returns (q uint8[n], scales f32[nblk]).

    The kernel writes whole blocks: ``nblk * 256`` bytes, the pad past ``n`` as zero codes.  A
    caller's ``q`` must hold that many (it is returned as given); without one the codes are
    allocated as whole blocks and the first ``n`` bytes returned as a view of them, so the result
    can be passed on to :func:`dequant_reduce_fp8` as it is.

    A NaN element encodes to NaN and is ignored in its block's amax; a block with an infinity gets
    an infinite scale and decodes to non-finite values throughout."""
    _dev_check(x, q, scales)
    n = x.numel()
    if n % 4:
        raise ValueError("quant_fp8: n must be a multiple of 4")
    nblk = (n + QBLOCK - 1) // QBLOCK
    own = q is None
    if own:
        q = torch.empty(nblk * QBLOCK, dtype=torch.uint8, device=x.device)
    if scales is None:
        scales = torch.empty(nblk, dtype=torch.float32, device=x.device)
    if q.dtype != torch.uint8 or scales.dtype != torch.float32:
        raise ValueError("quant_fp8: q must be uint8 and scales float32")
    if q.numel() < nblk * QBLOCK or scales.numel() < nblk:
        raise ValueError(f"quant_fp8: q needs whole blocks ({nblk * QBLOCK} bytes for n = {n}) and scales {nblk}")
    check(native.hip().mp4x_quant_fp8(int(dtype_of_torch(x.dtype)), x.data_ptr(), n, q.data_ptr(), scales.data_ptr(),
                                      stream_ptr(stream)), "mp4x_quant_fp8")
    return (q[:n] if own else q), scales


def quant_fp8_ef(x: torch.Tensor, resid: torch.Tensor, q: Optional[torch.Tensor] = None,
                 scales: Optional[torch.Tensor] = None, stream=None):
    """:func:`quant_fp8` with error feedback: quantises ``x + resid`` (one f32 add) and leaves in
    ``resid`` what the codes dropped, ``fma(-decode(code), scale, x + resid)``, for the next call.
    ``resid`` is f32 with ``x.numel()`` elements, 16-byte aligned, updated in place; ``x`` is not
    written.  Buffers and return value as :func:`quant_fp8`.

    A non-finite residual element is stored as 0: a NaN input resets its own element, a block with
    an infinity (its scale is infinite) resets the whole block.  With an all-``+0`` residual the
    codes and scales are :func:`quant_fp8`'s, except that an input of ``-0.0`` encodes as ``+0.0``."""
    _dev_check(x, resid, q, scales)
    n = x.numel()
    if n % 4:
        raise ValueError("quant_fp8_ef: n must be a multiple of 4")
    if resid.dtype != torch.float32 or resid.numel() != n:
        raise ValueError(f"quant_fp8_ef: resid must be float32 with {n} elements "
                         f"(got {resid.dtype}, {resid.numel()})")
    if resid.data_ptr() % 16:
        raise ValueError("quant_fp8_ef: resid must be 16-byte aligned")
    nblk = (n + QBLOCK - 1) // QBLOCK
    own = q is None
    if own:
        q = torch.empty(nblk * QBLOCK, dtype=torch.uint8, device=x.device)
    if scales is None:
        scales = torch.empty(nblk, dtype=torch.float32, device=x.device)
    if q.dtype != torch.uint8 or scales.dtype != torch.float32:
        raise ValueError("quant_fp8_ef: q must be uint8 and scales float32")
    if q.numel() < nblk * QBLOCK or scales.numel() < nblk:
        raise ValueError(f"quant_fp8_ef: q needs whole blocks ({nblk * QBLOCK} bytes for n = {n}) and scales {nblk}")
    check(native.hip().mp4x_quant_fp8_ef(int(dtype_of_torch(x.dtype)), x.data_ptr(), n, resid.data_ptr(), q.data_ptr(),
                                         scales.data_ptr(), stream_ptr(stream)), "mp4x_quant_fp8_ef")
    return (q[:n] if own else q), scales


def dequant_reduce_fp8(out: Optional[torch.Tensor], qs: Sequence[torch.Tensor], ss: Sequence[torch.Tensor], n: int,
                       accumulate: bool = False, q_out: Optional[torch.Tensor] = None,
                       s_out: Optional[torch.Tensor] = None, out_dtype=None, stream=None):
    """out[:n] (f32 / bf16 / f16) = [out +] sum_k dequant(qs[k], ss[k]), as the f32 chain
    ``acc = fma(code_k, scale_k, acc)`` in input order, stored with one rounding; with ``q_out`` /
    ``s_out`` the f32 accumulators (not the rounded ``out``) are re-quantised in the same pass.
    ``out`` may be None when only the re-quantised result is wanted.

    More than 8 inputs run as a chain of launches of up to 8.  The partial sums travel in f32 (in
    an f32 ``out``, or in a temporary when ``out`` is None), so the result is the one chain over
    all inputs, exactly.  A bf16 / f16 ``out`` carries them itself and so rounds once per launch of
    8; the re-quantised result then starts each later launch from that rounded value.

    Buffers are whole blocks (see :func:`quant_fp8`): ``q_out`` holds ``nblk * 256`` bytes, and
    with ``q_out`` every input must be backed by ``nblk * 256`` bytes whose pad past ``n`` is zero
    codes, as the quantiser writes them — the tensor itself or the allocation it is a view of (the
    ``n``-byte view :func:`quant_fp8` returns qualifies)."""
    nblk = (n + QBLOCK - 1) // QBLOCK
    if not qs or len(qs) != len(ss):
        raise ValueError("dequant_reduce_fp8: one scale tensor per code tensor")
    for q, s in zip(qs, ss):
        _dev_check(q, s)
        if q.numel() < n or s.numel() < nblk:
            raise ValueError("dequant_reduce_fp8: input too small")
        if q_out is not None and _room(q) < nblk * QBLOCK:
            raise ValueError(f"dequant_reduce_fp8: with q_out every input needs whole blocks "
                             f"({nblk * QBLOCK} bytes for n = {n})")
    if out is not None:
        _dev_check(out)
        if out.numel() < n:
            raise ValueError("dequant_reduce_fp8: out too small")
        dt = dtype_of_torch(out.dtype)
    else:
        dt = dtype_of_torch(out_dtype or torch.float32)
    if q_out is not None:
        _dev_check(q_out, s_out)
        if q_out.numel() < nblk * QBLOCK or s_out is None or s_out.numel() < nblk:
            raise ValueError(f"dequant_reduce_fp8: q_out needs whole blocks ({nblk * QBLOCK} bytes for n = {n}) "
                             f"and s_out {nblk}")
    if out is None and len(qs) > MAX_NIN:
        # the kernel keeps its partial sums in `out`: without one, chain through an f32 temporary
        # (every launch would otherwise start from zero and q_out hold the last launch's sum only)
        if n <= 0:
            return None
        out_k = torch.empty(n, dtype=torch.float32, device=qs[0].device)
        dt = dtype_of_torch(torch.float32)
    else:
        out_k = out
    lib = native.hip()
    done = 0
    first = True
    while done < len(qs):
        k = min(MAX_NIN, len(qs) - done)
        qp, k1 = ptr_array([t.data_ptr() for t in qs[done:done + k]])
        sp, k2 = ptr_array([t.data_ptr() for t in ss[done:done + k]])
        last = done + k == len(qs)
        check(lib.mp4x_dequant_reduce_fp8(int(dt), out_k.data_ptr() if out_k is not None else None, qp, sp, k, n,
                                          int(accumulate or not first),
                                          q_out.data_ptr() if (q_out is not None and last) else None,
                                          s_out.data_ptr() if (s_out is not None and last) else None,
                                          stream_ptr(stream)), "mp4x_dequant_reduce_fp8")
        done += k
        first = False
    return out


def dequant_fp8(q: torch.Tensor, scales: torch.Tensor, n: int, out: torch.Tensor, stream=None):
    return dequant_reduce_fp8(out, [q], [scales], n, stream=stream)


# ------------------------------------------------------------------ sparse (K4/K5/K7)
def key_owner(keys: torch.Tensor, p: int, stream=None):
    _dev_check(keys)
    n = keys.numel()
    dest = torch.empty(n, dtype=torch.int32, device=keys.device)
    hist = torch.zeros(p, dtype=torch.int32, device=keys.device)
    check(native.hip().mp4x_key_owner(keys.data_ptr(), n, p, dest.data_ptr(), hist.data_ptr(), stream_ptr(stream)),
          "mp4x_key_owner")
    return dest, hist


ZS_BLOCK = 256
ZS_MAX_CHUNKS = 256      # the chunk table is staged in LDS


def _zs_table(chunks, dev):
    starts = [int(c[0]) for c in chunks]
    lens = [int(c[1]) for c in chunks]
    bs = [0]
    for ln in lens:
        bs.append(bs[-1] + (ln + ZS_BLOCK - 1) // ZS_BLOCK)
    return torch.tensor(starts + lens + bs, dtype=torch.int64, device=dev), bs


def zs_encode(x: torch.Tensor, chunks=None, stream=None):
    """K6b lossless zero suppression of a flat tensor, per chunk ``(start, len)`` (default: whole).

    Returns ``(masks int64[4*nblk], counts int32[nblk], vals x.dtype[nnz], nnz per chunk, blk_start)``;
    chunk j owns blocks ``blk_start[j]:blk_start[j+1]`` and its non-zero words are the j-th
    consecutive run of ``vals``.  One device->host read (the per-chunk totals)."""
    _dev_check(x)
    x = x.reshape(-1)
    if chunks is None:
        chunks = [(0, x.numel())]
    if len(chunks) > ZS_MAX_CHUNKS:
        raise ValueError(f"zs_encode: at most {ZS_MAX_CHUNKS} chunks per call")
    dev = x.device
    table, bs = _zs_table(chunks, dev)
    nblk = bs[-1]
    total = sum(int(c[1]) for c in chunks)
    masks = torch.empty(4 * nblk, dtype=torch.int64, device=dev)
    counts = torch.empty(nblk, dtype=torch.int32, device=dev)
    offs = torch.zeros(nblk + 1, dtype=torch.int64, device=dev)
    vals = torch.empty(max(total, 1), dtype=x.dtype, device=dev)
    lib = native.hip()
    tb = lib.mp4x_zs_temp_bytes(nblk)
    temp = torch.empty(max(tb, 1), dtype=torch.uint8, device=dev)
    check(lib.mp4x_zs_encode(x.element_size(), x.data_ptr(), table.data_ptr(), len(chunks), nblk, masks.data_ptr(),
                             counts.data_ptr(), offs.data_ptr(), vals.data_ptr(), temp.data_ptr(), tb,
                             stream_ptr(stream)), "mp4x_zs_encode")
    at = offs[torch.tensor(bs, dtype=torch.int64, device=dev)].tolist() if nblk else [0] * len(bs)
    nnz = [at[j + 1] - at[j] for j in range(len(chunks))]
    return masks, counts, vals[:at[-1]], nnz, bs


def zs_decode(masks: torch.Tensor, counts: torch.Tensor, vals: torch.Tensor, chunks, out: torch.Tensor,
              stream=None):
    """Inverse of :func:`zs_encode`: chunk j (masks / counts / vals concatenated in chunk order)
    expands into ``out.view(-1)[start_j : start_j + len_j]``."""
    _dev_check(masks, counts, vals, out)
    if len(chunks) > ZS_MAX_CHUNKS:
        raise ValueError(f"zs_decode: at most {ZS_MAX_CHUNKS} chunks per call")
    dev = out.device
    table, bs = _zs_table(chunks, dev)
    nblk = bs[-1]
    if nblk == 0:
        return out
    if masks.numel() != 4 * nblk or counts.numel() != nblk:
        raise ValueError("zs_decode: masks / counts do not match the chunk table")
    if vals.element_size() != out.element_size():
        raise ValueError("zs_decode: vals / out word size differ")
    offs = torch.empty(nblk + 1, dtype=torch.int64, device=dev)
    lib = native.hip()
    tb = lib.mp4x_zs_temp_bytes(nblk)
    temp = torch.empty(max(tb, 1), dtype=torch.uint8, device=dev)
    check(lib.mp4x_zs_decode(out.element_size(), masks.data_ptr(), counts.data_ptr(),
                             vals.data_ptr() if vals.numel() else None, table.data_ptr(), len(chunks), nblk,
                             out.data_ptr(), offs.data_ptr(), temp.data_ptr(), tb, stream_ptr(stream)),
          "mp4x_zs_decode")
    return out


PACK_MAX_P = 2048


def partition_pack(keys: torch.Tensor, vals: Optional[torch.Tensor], p: int, want_perm: bool = False,
                   want_range: bool = False, stream=None):
    """Fused K4b stable partition by owner ``(uint64)key % p``.

    Returns ``(out_keys, out_vals, counts int64[p], perm)``; ``out_vals`` is None when
    ``vals`` is None, ``perm`` (source row of each slot) only with ``want_perm``.  Rows whose
    size is not a multiple of 16 bytes are packed with :func:`gather_rows` through ``perm``.
    ``want_range``: ``counts`` has two more entries, the smallest and largest key (0, 0 when
    empty), reduced inside the same kernels.
    """
    _dev_check(keys, vals)
    if keys.dtype != torch.int64:
        raise ValueError("partition_pack: keys must be int64")
    if not 1 <= p <= PACK_MAX_P:
        raise ValueError(f"partition_pack: p must be in [1, {PACK_MAX_P}]")
    n = keys.numel()
    dev = keys.device
    keys = keys.contiguous()
    row_bytes = 0
    fused_rows = False
    if vals is not None:
        if vals.shape[0] != n:
            raise ValueError("partition_pack: vals rows != keys")
        vals = vals.contiguous()
        row_bytes = (vals[0].numel() if n else 0) * vals.element_size()
        fused_rows = row_bytes % 16 == 0 and row_bytes > 0
    need_perm = want_perm or (vals is not None and not fused_rows)
    out_keys = torch.empty(n, dtype=torch.int64, device=dev)
    out_vals = torch.empty_like(vals) if vals is not None else None
    perm = torch.empty(n, dtype=torch.int64, device=dev) if need_perm else None
    counts = torch.empty(p + (2 if want_range else 0), dtype=torch.int64, device=dev)
    lib = native.hip()
    sb = lib.mp4x_partition_pack_scratch_bytes(n, p)
    scratch = torch.empty(max(sb, 1), dtype=torch.uint8, device=dev)
    check(lib.mp4x_partition_pack(keys.data_ptr(), vals.data_ptr() if fused_rows else None, n, row_bytes, p,
                                  out_keys.data_ptr(), out_vals.data_ptr() if fused_rows else None,
                                  perm.data_ptr() if perm is not None else None, counts.data_ptr(),
                                  counts.data_ptr() + 8 * p if want_range else None,
                                  scratch.data_ptr(), sb, stream_ptr(stream)), "mp4x_partition_pack")
    if vals is not None and not fused_rows and n:
        gather_rows(vals.view(n, -1), perm, out=out_vals.view(n, -1), stream=stream)
    return out_keys, out_vals, counts, perm


class PackCount(NamedTuple):
    """The first half of K4b (:func:`partition_count`): ``info`` = counts[p] + [min key, max
    key]; ``scratch`` holds the scan the second half (:func:`partition_scatter`) reads."""
    keys: torch.Tensor
    p: int
    info: torch.Tensor
    scratch: torch.Tensor


def partition_count(keys: torch.Tensor, p: int, stream=None) -> PackCount:
    """K4b's histogram + scan: rows per owner ``(uint64)key % p`` and the key range, with no rows
    moved yet (the caller can exchange the counts first)."""
    _dev_check(keys)
    if keys.dtype != torch.int64:
        raise ValueError("partition_count: keys must be int64")
    if not 1 <= p <= PACK_MAX_P:
        raise ValueError(f"partition_count: p must be in [1, {PACK_MAX_P}]")
    n = keys.numel()
    lib = native.hip()
    sb = lib.mp4x_partition_pack_scratch_bytes(n, p)
    scratch = torch.empty(max(sb, 1), dtype=torch.uint8, device=keys.device)
    info = torch.empty(p + 2, dtype=torch.int64, device=keys.device)
    check(lib.mp4x_partition_pack_count(keys.data_ptr(), n, p, info.data_ptr(), info.data_ptr() + 8 * p,
                                        scratch.data_ptr(), sb, stream_ptr(stream)), "mp4x_partition_pack_count")
    return PackCount(keys, p, info, scratch)


def partition_scatter(pc: PackCount, vals: Optional[torch.Tensor], out_vals_ptr: int, out_keys_ptr: int,
                      key_stride: int = 1, stream=None) -> None:
    """K4b's scatter after :func:`partition_count`: rows of ``vals`` (whole 16-byte vectors) to
    device address ``out_vals_ptr`` and keys to ``out_keys_ptr`` (``key_stride`` 2: the key half
    of 16-byte vectors) in stable owner-major order."""
    keys = pc.keys
    n = keys.numel()
    if n == 0:
        return
    _dev_check(keys, vals)
    rb = 0 if vals is None else vals[0].numel() * vals.element_size()
    if rb % 16 or (vals is not None and vals.shape[0] != n):
        raise ValueError("partition_scatter: rows of whole 16-byte vectors, one per key")
    check(native.hip().mp4x_partition_pack_scatter(keys.data_ptr(), vals.data_ptr() if vals is not None else None, n,
                                                   rb, pc.p, out_keys_ptr, int(key_stride),
                                                   out_vals_ptr if vals is not None else None, None,
                                                   pc.scratch.data_ptr(), pc.scratch.numel(), stream_ptr(stream)),
          "mp4x_partition_pack_scatter")


# ------------------------------------------------------------------ K9 expert-parallel token routing
MOE_MAX_EXPERTS = 2048
MOE_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


class RouteCount(NamedTuple):
    """The first half of K9's route (:func:`moe_route_count`): ``counts`` = assignments per expert
    [nb] + [negative ids, ids >= nb]; ``scratch`` holds the scan :func:`moe_route_scatter` reads."""
    ids: torch.Tensor
    nb: int
    counts: torch.Tensor
    scratch: torch.Tensor


def _moe_rows(fn: str, rows: torch.Tensor) -> Tuple[int, int]:
    """(elements, bytes) of one row of ``rows`` [R, ...]: f32 / bf16 / f16, whole 16-byte vectors."""
    if rows.dtype not in MOE_DTYPES:
        raise ValueError(f"{fn}: dtype {rows.dtype} is not float32 / bfloat16 / float16")
    width = 1
    for d in rows.shape[1:]:
        width *= int(d)
    rb = width * rows.element_size()
    if rows.dim() < 1 or rb == 0 or rb % 16:
        raise ValueError(f"{fn}: rows of {rb} bytes are not whole 16-byte vectors")
    return width, rb


def moe_route_count(ids: torch.Tensor, nb: int, stream=None) -> RouteCount:
    """K9's histogram + scan over the flattened (token, k) expert ids (int32 / int64): rows per
    expert ``0 <= id < nb`` and the number of negative and of too-large ids, with no rows moved
    yet (the caller can exchange the counts first)."""
    _dev_check(ids)
    if ids.dtype not in (torch.int32, torch.int64):
        raise ValueError("moe_route_count: ids must be int32 or int64")
    if not 1 <= nb <= MOE_MAX_EXPERTS:
        raise ValueError(f"moe_route_count: nb must be in [1, {MOE_MAX_EXPERTS}]")
    n = ids.numel()
    lib = native.hip()
    sb = lib.mp4x_moe_route_scratch_bytes(n, nb)
    scratch = torch.empty(max(sb, 1), dtype=torch.uint8, device=ids.device)
    counts = torch.empty(nb + 2, dtype=torch.int64, device=ids.device)
    check(lib.mp4x_moe_route_count(ids.data_ptr(), int(ids.dtype == torch.int64), n, nb, counts.data_ptr(),
                                   scratch.data_ptr(), sb, stream_ptr(stream)), "mp4x_moe_route_count")
    return RouteCount(ids, nb, counts, scratch)


def _moe_scatter_args(fn: str, rc: RouteCount, x: torch.Tensor, top_k: int, out_rows: torch.Tensor,
                      row_scale: Optional[torch.Tensor]) -> Tuple[int, int]:
    """What both K9 scatters ask of their arguments; (assignments, bytes of a row)."""
    n = rc.ids.numel()
    _dev_check(rc.ids, x, out_rows, row_scale)
    _, rb = _moe_rows(fn, x)
    if top_k < 1 or x.shape[0] * top_k != n:
        raise ValueError(f"{fn}: {x.shape[0]} rows x top_k {top_k} != {n} ids")
    if out_rows.dtype != x.dtype or tuple(out_rows.shape[1:]) != tuple(x.shape[1:]):
        raise ValueError(f"{fn}: out_rows dtype / row shape differ from x")
    if row_scale is not None and (row_scale.dtype != torch.float32 or row_scale.numel() != n):
        raise ValueError(f"{fn}: row_scale must be float32, one per assignment")
    return n, rb


def moe_route_scatter(rc: RouteCount, x: torch.Tensor, top_k: int, out_rows: torch.Tensor,
                      row_scale: Optional[torch.Tensor] = None, placed: Optional[int] = None,
                      stream=None, clip: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K9's scatter after :func:`moe_route_count`: ``slots`` int64[n], the position of assignment
    ``a = t * top_k + k`` in the stable sort by expert id (-1 where it is placed nowhere), and
    ``out_rows[slots[a]] = x[t]``, times ``row_scale[a]`` (float32, one rounding) when given.
    ``out_rows`` must hold every placed assignment (``rc.counts[:nb].sum()`` rows).

    ``clip`` (int64 ``[2 * nb]`` on the ids' device: ``keep[e]`` | its exclusive prefix): an expert
    capacity.  The ``pe``-th assignment of expert e stays iff ``pe < keep[e]``, at slot
    ``prefix[e] + pe``; the others get -1 and their rows are neither read nor written.  ``out_rows``
    must then hold ``keep.sum()`` rows, which the caller gives as ``placed`` (no sync here)."""
    ids = rc.ids
    n, rb = _moe_scatter_args("moe_route_scatter", rc, x, top_k, out_rows, row_scale)
    if clip is not None:
        _dev_check(ids, clip)
        if clip.dtype != torch.int64 or tuple(clip.shape) != (2 * rc.nb,) or not clip.is_contiguous():
            raise ValueError(f"moe_route_scatter: clip must be a contiguous int64 [{2 * rc.nb}] tensor")
    slots = torch.empty(n, dtype=torch.int64, device=ids.device)
    if n == 0:
        return slots
    # every computed slot is below the number of placed assignments (<= n): out_rows must hold
    # them.  ``placed``: that number when the caller has it on the host already (no sync here).
    if out_rows.shape[0] < n:
        if placed is None:
            placed = int(rc.counts[:rc.nb].sum()) if clip is None else int(clip[:rc.nb].sum())
        if out_rows.shape[0] < placed:
            raise ValueError("moe_route_scatter: out_rows holds fewer rows than are placed")
    if out_rows.shape[0] == 0:             # nothing is placed: the kernel still wants a valid address
        out_rows = torch.empty((1,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    head = (int(dtype_of_torch(x.dtype)), ids.data_ptr(), int(ids.dtype == torch.int64), x.data_ptr(),
            row_scale.data_ptr() if row_scale is not None else None, n, int(top_k), rb, rc.nb, out_rows.data_ptr(),
            slots.data_ptr())
    tail = (rc.scratch.data_ptr(), rc.scratch.numel(), stream_ptr(stream))
    if clip is None:
        check(native.hip().mp4x_moe_route_scatter(*head, *tail), "mp4x_moe_route_scatter")
    else:
        check(native.hip().mp4x_moe_route_scatter_clip(*head, clip.data_ptr(), *tail), "mp4x_moe_route_scatter_clip")
    return slots


def _moe_combine_args(fn: str, rows: torch.Tensor, slots: torch.Tensor, weights: Optional[torch.Tensor],
                      num_tokens: int, top_k: int, out: Optional[torch.Tensor]):
    """What both K9 combines ask of their rows, slots, weights and ``out`` (``[num_tokens, ...]`` in the
    rows' dtype; None: made here); (elements of a row, assignments, out)."""
    width, _ = _moe_rows(fn, rows)
    n = num_tokens * top_k
    if slots.dtype != torch.int64 or slots.numel() != n or top_k < 1:
        raise ValueError(f"{fn}: slots must be int64, num_tokens * top_k of them")
    if weights is not None and (weights.dtype != torch.float32 or weights.numel() != n):
        raise ValueError(f"{fn}: weights must be float32, one per assignment")
    if out is None:
        out = torch.empty((num_tokens,) + tuple(rows.shape[1:]), dtype=rows.dtype, device=rows.device)
    elif out.dtype != rows.dtype or tuple(out.shape) != (num_tokens,) + tuple(rows.shape[1:]):
        raise ValueError(f"{fn}: out dtype / shape mismatch")
    return width, n, out


def moe_combine(rows: torch.Tensor, slots: torch.Tensor, weights: Optional[torch.Tensor], num_tokens: int,
                top_k: int, out: Optional[torch.Tensor] = None, max_slot: Optional[int] = None, stream=None):
    """K9's combine: ``out[t] = sum over k, in k order, of weights[t, k] * rows[slots[t * top_k + k]]``
    (f32 accumulate from +0, product and sum rounded separately, slots < 0 skipped, one rounding to
    ``rows.dtype``).  ``max_slot`` is the largest slot when the caller already knows it (the plan's
    send total - 1); otherwise it is read back from ``slots`` for the bounds check."""
    _dev_check(rows, slots, weights, out)
    width, n, out = _moe_combine_args("moe_combine", rows, slots, weights, num_tokens, top_k, out)
    if n == 0:
        return out
    if max_slot is None:
        max_slot = int(slots.max())
    if max_slot >= rows.shape[0]:
        raise ValueError(f"moe_combine: slot {max_slot} past the {rows.shape[0]} rows")
    # (a call with nothing placed still hands the kernel a readable address)
    src = rows if rows.shape[0] else torch.zeros((1,) + tuple(rows.shape[1:]), dtype=rows.dtype, device=rows.device)
    check(native.hip().mp4x_moe_combine(int(dtype_of_torch(rows.dtype)), src.data_ptr(), slots.data_ptr(),
                                        weights.data_ptr() if weights is not None else None, num_tokens, int(top_k),
                                        width, out.data_ptr(), stream_ptr(stream)), "mp4x_moe_combine")
    return out


def _moe_share(fn: str, nb: int, cap) -> int:
    if isinstance(cap, bool) or not isinstance(cap, int) or cap < 1 or cap > (2 ** 31 - 1) // nb:
        raise ValueError(f"{fn}: the share {cap!r} is not an int in [1, {(2 ** 31 - 1) // nb}]")
    return cap


def moe_route_scatter_pad(rc: RouteCount, x: torch.Tensor, top_k: int, out_rows: torch.Tensor, cap: int,
                          row_scale: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
    """K9's scatter into the padded fixed-capacity layout after :func:`moe_route_count`: expert e
    owns rows ``[e * cap, (e + 1) * cap)`` of ``out_rows`` (exactly ``nb * cap`` rows).  The
    ``pe``-th assignment of expert e gets ``slots[a] = e * cap + pe`` iff ``pe < cap``, else -1 (as
    do a negative id and an id >= nb); ``out_rows[slots[a]] = x[t]`` (times ``row_scale[a]``), and
    every other row of ``out_rows`` is written as zeros, each row exactly once.  Every shape is
    known before the ids are: nothing is read back, nothing is copied to the device."""
    ids = rc.ids
    cap = _moe_share("moe_route_scatter_pad", rc.nb, cap)
    n, rb = _moe_scatter_args("moe_route_scatter_pad", rc, x, top_k, out_rows, row_scale)
    if out_rows.shape[0] != rc.nb * cap:
        raise ValueError(f"moe_route_scatter_pad: out_rows holds {out_rows.shape[0]} rows, not {rc.nb} x {cap}")
    slots = torch.empty(n, dtype=torch.int64, device=ids.device)
    check(native.hip().mp4x_moe_route_scatter_pad(
        int(dtype_of_torch(x.dtype)), ids.data_ptr() if n else None, int(ids.dtype == torch.int64),
        x.data_ptr() if n else None, row_scale.data_ptr() if row_scale is not None and n else None, n, int(top_k), rb,
        rc.nb, cap, out_rows.data_ptr(), slots.data_ptr() if n else None, rc.scratch.data_ptr() if n else None,
        rc.scratch.numel() if n else 0, stream_ptr(stream)), "mp4x_moe_route_scatter_pad")
    return slots


def moe_pad_counts(rc: RouteCount, cap: int, group: Optional[int] = None, group_pad: Optional[int] = None,
                   kept: Optional[torch.Tensor] = None, stream=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(kept, dropped)`` of the padded layout after :func:`moe_route_count`: ``kept[e] =
    min(count of e, cap)`` and ``dropped`` int64 [3] = assignments past their share | negative ids |
    ids >= nb, both on the ids' device and never read here.  ``group`` / ``group_pad``: ``kept`` is
    laid out ``[nb / group, group_pad]`` (zero padding) instead of ``[nb]``; ``kept``: write there."""
    ids = rc.ids
    cap = _moe_share("moe_pad_counts", rc.nb, cap)
    el = rc.nb if group is None else int(group)
    el_pad = el if group_pad is None else int(group_pad)
    if el < 1 or rc.nb % el or el_pad < el:
        raise ValueError(f"moe_pad_counts: groups of {el} (padded to {el_pad}) do not tile {rc.nb} experts")
    size = rc.nb // el * el_pad
    if kept is None:
        kept = torch.empty(size, dtype=torch.int64, device=ids.device)
    _dev_check(ids, kept)
    if kept.dtype != torch.int64 or kept.numel() != size:
        raise ValueError(f"moe_pad_counts: kept must be int64 [{size}]")
    dropped = torch.empty(3, dtype=torch.int64, device=ids.device)
    n = ids.numel()
    check(native.hip().mp4x_moe_pad_counts(n, rc.nb, cap, el, el_pad, kept.data_ptr(), dropped.data_ptr(),
                                           rc.scratch.data_ptr() if n else None, rc.scratch.numel() if n else 0,
                                           stream_ptr(stream)), "mp4x_moe_pad_counts")
    return kept, dropped


def moe_combine_rows(rows: torch.Tensor, slots: torch.Tensor, weights: Optional[torch.Tensor], num_tokens: int,
                     top_k: int, out: Optional[torch.Tensor] = None, stream=None):
    """:func:`moe_combine` over the padded layout: the slots index ``rows`` anywhere (the scatter
    that made them bounds them by ``rows.shape[0]`` = nb * cap by construction), so nothing is read
    back for a bounds check.  Rows no slot names are never read."""
    _dev_check(rows, slots, weights, out)
    width, n, out = _moe_combine_args("moe_combine_rows", rows, slots, weights, num_tokens, top_k, out)
    if rows.shape[0] < 1:
        raise ValueError("moe_combine_rows: no rows")
    if n == 0:
        return out
    check(native.hip().mp4x_moe_combine_rows(int(dtype_of_torch(rows.dtype)), rows.data_ptr(), rows.shape[0],
                                             slots.data_ptr(), weights.data_ptr() if weights is not None else None,
                                             num_tokens, int(top_k), width, out.data_ptr(), stream_ptr(stream)),
          "mp4x_moe_combine_rows")
    return out


def moe_priority_mask(rc: RouteCount, priority: torch.Tensor, limit, out: Optional[torch.Tensor] = None,
                      stream=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """K15, the per-expert top-S select after :func:`moe_route_count`: ``(ids_out, masked)``.
    ``ids_out[a] = rc.ids[a]`` for the ``limit[e]`` assignments of every expert e with the largest
    ``(gate key of priority[a], -a)`` (float order with -0 == +0, a positive NaN above +inf, a negative
    one below -inf; ties to the lower a), -1 for the expert's other assignments; a negative id and an
    id >= nb pass through.  ``priority``: float32, one per assignment.  ``limit``: an int >= 0 for every
    expert, or an int64 ``[nb]`` tensor on the ids' device (a negative entry counts as 0).  ``masked``:
    int64 ``[1]`` on the device, the assignments turned into -1.  ``out``: write there (the ids' dtype
    and size, not the ids themselves).  Nothing is read back and the result is identical run to run."""
    ids = rc.ids
    _dev_check(ids, priority, out, limit if isinstance(limit, torch.Tensor) else None)
    n = ids.numel()
    if priority.dtype != torch.float32 or priority.numel() != n:
        raise ValueError(f"moe_priority_mask: priority must be float32, one per assignment ({n})")
    if isinstance(limit, torch.Tensor):
        if limit.dtype != torch.int64 or tuple(limit.shape) != (rc.nb,):
            raise ValueError(f"moe_priority_mask: a limit tensor must be int64 [{rc.nb}]")
        scalar, vec = 0, limit.data_ptr()
    else:
        if isinstance(limit, bool) or not isinstance(limit, int) or not 0 <= limit < 2 ** 63:
            raise ValueError(f"moe_priority_mask: the limit {limit!r} is not an int >= 0 or an int64 [{rc.nb}] tensor")
        scalar, vec = limit, None
    if out is None:
        out = torch.empty_like(ids)
    elif out.dtype != ids.dtype or out.numel() != n or out.data_ptr() == ids.data_ptr() and n:
        raise ValueError("moe_priority_mask: out must have the ids' dtype and size and be another tensor")
    lib = native.hip()
    sb = lib.mp4x_moe_priority_scratch_bytes(n, rc.nb)
    scratch = torch.empty(max(sb, 1), dtype=torch.uint8, device=ids.device)
    masked = torch.empty(1, dtype=torch.int64, device=ids.device)
    check(lib.mp4x_moe_priority_mask(ids.data_ptr() if n else None, int(ids.dtype == torch.int64),
                                     priority.data_ptr() if n else None, n, rc.nb, scalar, vec,
                                     rc.scratch.data_ptr() if n else None, rc.scratch.numel() if n else 0,
                                     out.data_ptr() if n else None, masked.data_ptr(), scratch.data_ptr(), sb,
                                     stream_ptr(stream)), "mp4x_moe_priority_mask")
    return out, masked


MOE_COMBINE_BWD_MAX_TOP_K = 16       # csrc/kernels/moe.hip: kMoeBwdMaxK


def moe_combine_backward(g: torch.Tensor, rows: torch.Tensor, slots: torch.Tensor, weights: torch.Tensor,
                         num_tokens: int, top_k: int, out=None, pad=None, max_slot: Optional[int] = None, stream=None):
    """K11, both gradients of :func:`moe_combine` in one pass over its output gradient ``g``
    [T, ...]: ``(g_rows, g_weights)``.  ``rows`` are the rows the combine read (slot order).  Per
    assignment ``a = t * top_k + k`` with ``s = slots[a] >= 0``: ``g_rows[s] = weights[a] * g[t]``
    (one multiply, one rounding: the bits of :func:`moe_route_scatter` with ``row_scale``) and
    ``g_weights[a] = sum_h g[t, h] * rows[s, h]`` in float32, in an order fixed by the dtype and the
    row width; with ``s < 0`` no row is read or written and ``g_weights[a] = +0``.  Every slot value
    appears at most once; a row of ``g_rows`` no slot names stays as it was.

    ``out``: ``(g_rows, g_weights)`` to write instead of new tensors.  ``pad = (rc, cap)``, the
    :class:`RouteCount` and the share of the :func:`moe_route_scatter_pad` that made ``slots``: the
    padded layout, ``rc.nb * cap`` rows, where the pad rows of every expert block are written as
    zeros as that scatter does (every row written exactly once) and nothing is read back.  Without
    ``pad``, ``max_slot`` is the largest slot when the caller knows it (else it is read back)."""
    fn = "moe_combine_backward"
    _dev_check(g, rows, slots, weights)
    width, _ = _moe_rows(fn, rows)
    if isinstance(top_k, bool) or not isinstance(top_k, int) or not 1 <= top_k <= MOE_COMBINE_BWD_MAX_TOP_K:
        raise ValueError(f"{fn}: top_k {top_k!r} is not an int in [1, {MOE_COMBINE_BWD_MAX_TOP_K}]")
    n = num_tokens * top_k
    if n > (2 ** 31 - 1) // 2:
        raise ValueError(f"{fn}: {num_tokens} tokens x top_k {top_k} is past the routed limit")
    if g.dtype != rows.dtype or tuple(g.shape) != (num_tokens,) + tuple(rows.shape[1:]):
        raise ValueError(f"{fn}: g must be {(num_tokens,) + tuple(rows.shape[1:])} in the rows' dtype")
    # (K11's own slot and weight checks stay inlined: through _moe_combine_args a 13 us call measured 0.3 us slower)
    if slots.dtype != torch.int64 or slots.numel() != n:
        raise ValueError(f"{fn}: slots must be int64, num_tokens * top_k of them")
    if weights is None or weights.dtype != torch.float32 or weights.numel() != n:
        raise ValueError(f"{fn}: weights must be float32, one per assignment")
    if pad is not None:
        rc, cap = pad
        cap = _moe_share(fn, rc.nb, cap)
        if rc.ids.numel() != n or rows.shape[0] != rc.nb * cap:
            raise ValueError(f"{fn}: the padded layout has {rc.nb} x {cap} rows for {rc.ids.numel()} assignments")
        _dev_check(g, rc.scratch)
    if out is None:
        out = (torch.empty_like(rows), torch.empty((num_tokens, top_k), dtype=torch.float32, device=g.device))
    g_rows, g_weights = out
    _dev_check(g, g_rows, g_weights)
    if g_rows.dtype != rows.dtype or g_rows.shape != rows.shape:
        raise ValueError(f"{fn}: out[0] dtype / shape differ from the rows'")
    if g_weights.dtype != torch.float32 or g_weights.numel() != n:
        raise ValueError(f"{fn}: out[1] must be float32, one per assignment")
    lib, dt = native.hip(), int(dtype_of_torch(rows.dtype))
    if pad is not None:
        check(lib.mp4x_moe_combine_backward_pad(
            dt, g.data_ptr() if n else None, rows.data_ptr(), slots.data_ptr() if n else None,
            weights.data_ptr() if n else None, num_tokens, top_k, width, n, rc.nb, cap,
            rc.scratch.data_ptr() if n else None, rc.scratch.numel() if n else 0, g_rows.data_ptr(),
            g_weights.data_ptr() if n else None, stream_ptr(stream)), "mp4x_moe_combine_backward_pad")
        return g_rows, g_weights
    if n == 0:
        return g_rows, g_weights
    if max_slot is None:
        max_slot = int(slots.max())
    if max_slot >= rows.shape[0]:
        raise ValueError(f"{fn}: slot {max_slot} past the {rows.shape[0]} rows")
    src, dst = rows, g_rows
    if rows.shape[0] == 0:                 # nothing is placed: the kernel still wants valid addresses
        src = torch.zeros((2,) + tuple(rows.shape[1:]), dtype=rows.dtype, device=rows.device)
        src, dst = src[:1], src[1:]
    check(lib.mp4x_moe_combine_backward(dt, g.data_ptr(), src.data_ptr(), src.shape[0], slots.data_ptr(),
                                        weights.data_ptr(), num_tokens, top_k, width, dst.data_ptr(),
                                        g_weights.data_ptr(), stream_ptr(stream)), "mp4x_moe_combine_backward")
    return g_rows, g_weights


MOE_GATE_MAX_TOP_K = 16


def _gate_shape(fn: str, logits: torch.Tensor, top_k) -> Tuple[int, int, int]:
    """(T, E, K) of a K10 call, checked as csrc/kernels/moe_gate.hip checks them."""
    if logits.dim() != 2 or logits.dtype not in MOE_DTYPES:
        raise ValueError(f"{fn}: logits must be [T, E] in float32 / bfloat16 / float16")
    T, E = int(logits.shape[0]), int(logits.shape[1])
    if not 1 <= E <= MOE_MAX_EXPERTS:
        raise ValueError(f"{fn}: E = {E} is not in [1, {MOE_MAX_EXPERTS}]")
    if isinstance(top_k, bool) or not isinstance(top_k, int) or not 1 <= top_k <= min(E, MOE_GATE_MAX_TOP_K):
        raise ValueError(f"{fn}: top_k {top_k!r} is not an int in [1, min(E, {MOE_GATE_MAX_TOP_K})]")
    if T * top_k > (2 ** 31 - 1) // 2:
        raise ValueError(f"{fn}: {T} tokens x top_k {top_k} is past the routed limit")
    return T, E, top_k


def _ptr(t: Optional[torch.Tensor], on=True):
    """The address of ``t``, None for no tensor or with ``on`` false (a call with no token passes none)."""
    return t.data_ptr() if (t is not None and on) else None


def _gate_outputs(fn: str, logits: torch.Tensor, want, out, names: str):
    """The tensors a gate forward writes: new ones of ``want`` (a ``(shape, dtype)`` each, None where
    the call has none), or ``out`` checked against it; an entry the call has none for is not looked at."""
    if out is None:
        return tuple(None if w is None else torch.empty(w[0], dtype=w[1], device=logits.device) for w in want)
    out = tuple(out)
    if len(out) != len(want) or any(w is not None and (not isinstance(t, torch.Tensor) or tuple(t.shape) != w[0]
                                                       or t.dtype != w[1] or not t.is_contiguous())
                                    for t, w in zip(out, want)):
        raise ValueError(f"{fn}: out must be ({names}) of the call's shapes and dtypes")
    _dev_check(logits, *(t for t, w in zip(out, want) if w is not None))
    return out


def _gate_scratch(scratch_bytes, dt: int, T: int, E: int, stats: bool, device):
    """(tensor, bytes) of the statistics' scratch by the entry's own ``scratch_bytes``; (None, 0)
    without ``stats``."""
    if not stats:
        return None, 0
    sb = scratch_bytes(dt, T, E)
    return torch.empty(max(sb, 1), dtype=torch.uint8, device=device), sb


def _gate_backward(fn: str, logits, lse, ids, sigmoid: bool, g_weights, g_lse, g_prob_sum, out, call):
    """What both gate backwards do around their C entry: the tensor checks (the softmax score needs
    ``lse``, the sigmoid score has none), ``out``, nothing to do for no token, then
    ``call((dtype, logits, lse, ids, ids_are_i64, T, E, K), (g_weights, g_lse, g_prob_sum, out))`` with
    the addresses in the entry's order."""
    _dev_check(logits, lse, ids, g_weights, g_lse, g_prob_sum, out)
    if ids.dim() != 2 or ids.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{fn}: ids must be [T, K] in int32 or int64")
    T, E, K = _gate_shape(fn, logits, int(ids.shape[1]))
    if ids.shape[0] != T:
        raise ValueError(f"{fn}: {ids.shape[0]} rows of ids for {T} rows of logits")
    for name, t, shape in (("lse", lse, (T,)), ("g_weights", g_weights, (T, K)), ("g_lse", g_lse, (T,)),
                           ("g_prob_sum", g_prob_sum, (E,))):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != shape):
            raise ValueError(f"{fn}: {name} must be float32 {list(shape)}")
    if not sigmoid and lse is None:
        raise ValueError(f"{fn}: lse is missing")
    if sigmoid and (lse is not None or g_lse is not None):
        raise ValueError(f"{fn}: the sigmoid score has no lse")
    if out is None:
        out = torch.empty_like(logits)
    elif out.dtype != logits.dtype or out.shape != logits.shape:
        raise ValueError(f"{fn}: out dtype / shape differ from the logits'")
    if T:
        call((int(dtype_of_torch(logits.dtype)), logits.data_ptr(), _ptr(lse), ids.data_ptr(), int(ids.dtype == torch.int64),
              T, E, K), (_ptr(g_weights), _ptr(g_lse), _ptr(g_prob_sum), out.data_ptr()))
    return out


def moe_gate_topk(logits: torch.Tensor, top_k: int, renormalize: bool = False, ids_dtype=torch.int64,
                  stats: bool = False, stream=None, out=None):
    """K10's forward over ``logits`` [T, E]: ``(weights, ids, lse, prob_sum, counts)``.  ``ids``
    [T, K] are the first K experts of a token in the order (logit descending, index ascending),
    ``weights`` float32 [T, K] their softmax probabilities (divided by their sum with
    ``renormalize``), ``lse`` float32 [T] the row's log-sum-exp.  With ``stats``: ``prob_sum``
    float32 [E], the probabilities summed over the tokens in a fixed order, and ``counts`` int64 [E],
    the tokens routed to every expert; both None without.  ``out``: the five tensors to write
    (the last two None without ``stats``) instead of new ones.  Nothing is read back."""
    fn = "moe_gate_topk"
    _dev_check(logits)
    T, E, K = _gate_shape(fn, logits, top_k)
    if ids_dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{fn}: ids_dtype must be int32 or int64")
    want = (((T, K), torch.float32), ((T, K), ids_dtype), ((T,), torch.float32), ((E,), torch.float32) if stats else None,
            ((E,), torch.int64) if stats else None)
    out = _gate_outputs(fn, logits, want, out, "weights, ids, lse, prob_sum, counts")
    weights, ids, lse = out[:3]
    prob_sum, counts = out[3:] if stats else (None, None)
    lib = native.hip()
    dt = int(dtype_of_torch(logits.dtype))
    scratch, sb = _gate_scratch(lib.mp4x_moe_gate_scratch_bytes, dt, T, E, stats, logits.device)
    if T == 0 and not stats:
        return weights, ids, lse, None, None
    check(lib.mp4x_moe_gate_topk(dt, logits.data_ptr() if T else None, T, E, K, int(bool(renormalize)),
                                 weights.data_ptr() if T else None, ids.data_ptr() if T else None,
                                 int(ids_dtype == torch.int64), lse.data_ptr() if T else None,
                                 prob_sum.data_ptr() if stats else None, counts.data_ptr() if stats else None,
                                 scratch.data_ptr() if stats else None, sb, stream_ptr(stream)), "mp4x_moe_gate_topk")
    return weights, ids, lse, prob_sum, counts


def moe_gate_backward(logits: torch.Tensor, lse: torch.Tensor, ids: torch.Tensor, renormalize: bool = False,
                      g_weights: Optional[torch.Tensor] = None, g_lse: Optional[torch.Tensor] = None,
                      g_prob_sum: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, stream=None):
    """K10's backward: the gradient of ``logits`` (their dtype, one rounding) from the saved
    ``logits``, ``lse`` and ``ids`` of :func:`moe_gate_topk` and the gradients of ``weights`` [T, K],
    ``lse`` [T] and ``prob_sum`` [E], all float32, each None for zeros."""
    return _gate_backward(
        "moe_gate_backward", logits, lse, ids, False, g_weights, g_lse, g_prob_sum, out,
        lambda head, tail: check(native.hip().mp4x_moe_gate_backward(*head, int(bool(renormalize)), *tail, stream_ptr(stream)),
                                 "mp4x_moe_gate_backward"))


MOE_GATE_MAX_GROUPS = 32
MOE_GATE_SCORES = ("softmax", "sigmoid")          # the C ABI's score argument is the index


def gate_group_args(where: str, E: int, K: int, score, n_group, topk_group, scale, max_groups: Optional[int] = None,
                    names=("n_group", "topk_group", "scale", "E")) -> Tuple[int, int, float]:
    """``(n_group, topk_group, scale)`` of the group-limited gate over E experts with top K, checked
    (``topk_group`` None is ``n_group``): the one check behind ``route_topk_grouped``, the layer's
    constructor and the K13 wrappers.  ``where`` opens the message and ``names`` are the caller's names
    of its arguments; ``max_groups`` is the kernel's limit, None where there is none.  Loads nothing."""
    gn, kn, sn, en = names
    if score not in MOE_GATE_SCORES:
        raise ValueError(f"{where}score {score!r} is not 'softmax' or 'sigmoid'")
    if (isinstance(n_group, bool) or not isinstance(n_group, int) or n_group < 1 or E % n_group
            or (max_groups is not None and n_group > max_groups)):
        what = "a positive int" if max_groups is None else f"an int in [1, {max_groups}]"
        raise ValueError(f"{where}{gn} {n_group!r} is not {what} that divides {en} = {E}")
    if topk_group is None:
        topk_group = n_group
    if isinstance(topk_group, bool) or not isinstance(topk_group, int) or not 1 <= topk_group <= n_group:
        raise ValueError(f"{where}{kn} {topk_group!r} is not an int in [1, {gn} = {n_group}]")
    if K > topk_group * (E // n_group):
        raise ValueError(f"{where}top_k {K} is more than the {topk_group} x {E // n_group} experts of the chosen groups")
    scale = float(scale)
    if not (scale > 0.0 and scale != float("inf")):
        raise ValueError(f"{where}{sn} {scale!r} is not finite and positive")
    return n_group, topk_group, scale


def _gate_group_args(fn: str, E: int, K: int, score, n_group, topk_group, scale) -> Tuple[int, int, int, float]:
    """(score index, n_group, topk_group, scale) of a K13 call, checked as csrc/kernels/moe_gate_group.hip
    checks them."""
    n_group, topk_group, scale = gate_group_args(f"{fn}: ", E, K, score, n_group, topk_group, scale, MOE_GATE_MAX_GROUPS)
    return MOE_GATE_SCORES.index(score), n_group, topk_group, scale


def moe_gate_group_topk(logits: torch.Tensor, top_k: int, score: str = "sigmoid", bias: Optional[torch.Tensor] = None,
                        n_group: int = 1, topk_group: Optional[int] = None, renormalize: bool = False,
                        scale: float = 1.0, ids_dtype=torch.int64, stats: bool = False, stream=None, out=None):
    """K13's forward over ``logits`` [T, E]: ``(weights, ids, lse, prob_sum, counts, group_ids)``.
    The score s is the softmax or ``1 / (1 + exp(-l))``; a token first takes the ``topk_group`` of
    the ``n_group`` contiguous expert groups with the largest sum of their two largest selection
    scores ``s + bias`` (``group_ids`` int32 [T, topk_group], in that order), then its K experts
    inside them, in the order (selection score descending, index ascending; the logits' own order
    without a bias).  ``weights`` float32 [T, K] are the chosen s (not s + bias), divided by their
    sum with ``renormalize``, times ``scale``.  ``lse`` is None for the sigmoid score; ``prob_sum``
    and ``counts`` are None without ``stats``.  ``out``: the six tensors to write (None where the
    call has none) instead of new ones.  Nothing is read back."""
    fn = "moe_gate_group_topk"
    _dev_check(logits, bias)
    T, E, K = _gate_shape(fn, logits, top_k)
    sc, Gr, Kg, scale = _gate_group_args(fn, E, K, score, n_group, topk_group, scale)
    if ids_dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{fn}: ids_dtype must be int32 or int64")
    if bias is not None and (bias.dtype != torch.float32 or tuple(bias.shape) != (E,) or not bias.is_contiguous()):
        raise ValueError(f"{fn}: bias must be contiguous float32 [{E}]")
    want = (((T, K), torch.float32), ((T, K), ids_dtype), ((T,), torch.float32) if sc == 0 else None,
            ((E,), torch.float32) if stats else None, ((E,), torch.int64) if stats else None, ((T, Kg), torch.int32))
    out = _gate_outputs(fn, logits, want, out, "weights, ids, lse, prob_sum, counts, group_ids")
    if any(w is None and t is not None for t, w in zip(out, want)):
        raise ValueError(f"{fn}: out must be None where the call has none")
    weights, ids, lse, prob_sum, counts, group_ids = out
    lib = native.hip()
    dt = int(dtype_of_torch(logits.dtype))
    scratch, sb = _gate_scratch(lib.mp4x_moe_gate_group_scratch_bytes, dt, T, E, stats, logits.device)
    if T == 0 and not stats:
        return out
    check(lib.mp4x_moe_gate_group_topk(dt, _ptr(logits, T), bias.data_ptr() if bias is not None else None, T, E, K, Gr, Kg, sc,
                                       int(bool(renormalize)), scale, _ptr(weights, T), _ptr(ids, T),
                                       int(ids_dtype == torch.int64), _ptr(group_ids, T), _ptr(lse, T),
                                       prob_sum.data_ptr() if stats else None, counts.data_ptr() if stats else None,
                                       scratch.data_ptr() if stats else None, sb, stream_ptr(stream)),
          "mp4x_moe_gate_group_topk")
    return out


def moe_gate_group_backward(logits: torch.Tensor, lse: Optional[torch.Tensor], ids: torch.Tensor, score: str = "sigmoid",
                            renormalize: bool = False, scale: float = 1.0, g_weights: Optional[torch.Tensor] = None,
                            g_lse: Optional[torch.Tensor] = None, g_prob_sum: Optional[torch.Tensor] = None,
                            out: Optional[torch.Tensor] = None, stream=None):
    """K13's backward: the gradient of ``logits`` (their dtype, one rounding) from the saved
    ``logits``, ``ids`` and (softmax) ``lse`` of :func:`moe_gate_group_topk` and the gradients of
    ``weights`` [T, K], ``lse`` [T] and ``prob_sum`` [E], all float32, each None for zeros.  The
    sigmoid score has no ``lse``: ``lse`` and ``g_lse`` must be None."""
    fn = "moe_gate_group_backward"
    sc, _, _, scale = _gate_group_args(fn, 1, 1, score, 1, 1, scale)      # one group of one expert: the score and the scale
    return _gate_backward(
        fn, logits, lse, ids, sc == 1, g_weights, g_lse, g_prob_sum, out,
        lambda head, tail: check(native.hip().mp4x_moe_gate_group_backward(*head, sc, int(bool(renormalize)), scale, *tail,
                                                                           stream_ptr(stream)), "mp4x_moe_gate_group_backward"))


# int64 key sorts: rocPRIM's own dispatch (block sort + merge passes below 1 M items, whatever the
# key width) or forced onesweep (csrc/kernels/sparse.hip OnesweepSort: ~27 us per 8-bit pass at
# 200 k items).  Measured on MI355X (profiles/r6/sparse/sort_ab.jsonl): onesweep wins at <= 16 bits
# from 200 k items and at <= 40 bits from ~1 M items (0.107 vs 0.199 ms at 1 M x 24 bits).
# MP4X_SORT_ALGO=rocprim | onesweep pins one.
SORT_ALGO = os.environ.get("MP4X_SORT_ALGO", "auto").lower()


def sort_algo(n: int, bits: int) -> int:
    """0 = rocPRIM's dispatch, 1 = onesweep, for ``n`` int64 keys over ``bits`` bits."""
    if SORT_ALGO in ("rocprim", "onesweep"):
        return int(SORT_ALGO == "onesweep")
    return 1 if bits <= 16 or (n >= 400_000 and bits <= 40) else 0


def sort_pairs(keys: torch.Tensor, idx: Optional[torch.Tensor] = None, end_bit: Optional[int] = None, stream=None,
               algo: Optional[int] = None):
    """Stable radix sort of int64 (or int32) keys with an int64 payload (default arange).
    ``algo`` (int64 keys): 0 = rocPRIM's choice, 1 = onesweep; None = by key width."""
    _dev_check(keys)
    n = keys.numel()
    if idx is None:
        idx = torch.arange(n, dtype=torch.int64, device=keys.device)
    ko = torch.empty_like(keys)
    io = torch.empty_like(idx)
    lib = native.hip()
    is32 = keys.dtype == torch.int32
    tb = lib.mp4x_sort_pairs_temp_bytes(n, int(is32))
    temp = torch.empty(max(tb, 1), dtype=torch.uint8, device=keys.device)
    eb = end_bit if end_bit is not None else (32 if is32 else 64)
    if is32:
        check(lib.mp4x_sort_pairs_i32key(keys.data_ptr(), ko.data_ptr(), idx.data_ptr(), io.data_ptr(), n, 0, eb,
                                         temp.data_ptr(), tb, stream_ptr(stream)), "mp4x_sort_pairs")
        return ko, io
    if algo is None:
        algo = sort_algo(n, eb)
    check(lib.mp4x_sort_pairs_i64(keys.data_ptr(), ko.data_ptr(), idx.data_ptr(), io.data_ptr(), n, 0, eb, int(algo),
                                  temp.data_ptr(), tb, stream_ptr(stream)), "mp4x_sort_pairs")
    return ko, io


def run_starts(sorted_keys: torch.Tensor, stream=None):
    """Start index of every run of equal keys; returns (starts[n] buffer, nruns device scalar)."""
    _dev_check(sorted_keys)
    n = sorted_keys.numel()
    dev = sorted_keys.device
    starts = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    nruns = torch.zeros(1, dtype=torch.int64, device=dev)
    flags = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    lib = native.hip()
    tb = lib.mp4x_rle_temp_bytes(max(n, 1))
    temp = torch.empty(max(tb, 1), dtype=torch.uint8, device=dev)
    check(lib.mp4x_run_starts(sorted_keys.data_ptr(), n, starts.data_ptr(), nruns.data_ptr(), flags.data_ptr(),
                              temp.data_ptr(), tb, stream_ptr(stream)), "mp4x_run_starts")
    return starts, nruns


def stage_split(keys: torch.Tensor, vals: Optional[torch.Tensor], vals_ptr: int, keys16_ptr: int,
                stream=None) -> None:
    """Sparse exchange staging (see mp4x/parallel/sparse.py): rows of ``vals`` [n, ...] copied to
    device address ``vals_ptr`` and ``keys`` [n] written as 16-byte {key, 0} vectors at
    ``keys16_ptr``, one launch (csrc/kernels/copy.hip k_stage_split)."""
    n = keys.shape[0]
    if n == 0:
        return
    _dev_check(keys, vals)
    rb = 0 if vals is None else vals[0].numel() * vals.element_size()
    if keys.dtype != torch.int64 or not keys.is_contiguous() or rb % 16 or \
            (vals is not None and (vals.shape[0] != n or not vals.is_contiguous())):
        raise ValueError("stage_split: contiguous int64 keys[n], rows of whole 16-byte vectors")
    check(native.hip().mp4x_stage_split(keys.data_ptr(), vals.data_ptr() if vals is not None else None, n, rb,
                                        vals_ptr if rb else None, keys16_ptr, stream_ptr(stream)), "mp4x_stage_split")


def keys_from16(k16: torch.Tensor, stream=None) -> torch.Tensor:
    """int64 keys of a uint8 [m * 16] region of {key, 0} vectors (the inverse of the key half of
    :func:`stage_split`)."""
    _dev_check(k16)
    m = k16.numel() // 16
    keys = torch.empty(m, dtype=torch.int64, device=k16.device)
    if m:
        check(native.hip().mp4x_keys_from16(k16.data_ptr(), m, keys.data_ptr(), stream_ptr(stream)), "mp4x_keys_from16")
    return keys


def hash_rbk_supported(dtype: torch.dtype, op: int) -> bool:
    """Does the hash reduce-by-key (K5h, csrc/kernels/sparse_hash.hip) serve (dtype, op)?"""
    try:
        dt = dtype_of_torch(dtype)
    except Exception:   # noqa: BLE001
        return False
    return bool(native.hip().mp4x_hash_rbk_supported(int(dt), int(op)))


def hash_reduce_by_key(keys: torch.Tensor, vals: torch.Tensor, op: int, stream=None):
    """K5h (csrc/kernels/sparse_hash.hip): (unique_keys, reduced_rows, counts) with the keys in
    hash-table order — one hashing pass finds the runs and links each key's rows (instead of the
    sort path's radix sort of the 64-bit keys), and lane groups combine every key's rows in input
    order (runs up to 64 rows: the same values, bit for bit, as :func:`reduce_by_key`).  Every
    reduction except the FIRST rule (then use :func:`reduce_by_key`)."""
    _dev_check(keys, vals)
    n = keys.numel()
    if keys.dtype != torch.int64 or vals.dim() not in (1, 2) or vals.shape[0] != n:
        raise ValueError("hash_reduce_by_key: int64 keys[n] and vals[n] / vals[n, dim]")
    if not hash_rbk_supported(vals.dtype, op):
        raise ValueError(f"hash_reduce_by_key: {vals.dtype} op {op} not supported")
    dev = keys.device
    dim = 1 if vals.dim() == 1 else int(vals.shape[1])
    lib = native.hip()
    sb = lib.mp4x_hash_rbk_scratch_bytes(n)
    scratch = torch.empty(sb + 256, dtype=torch.uint8, device=dev)
    sp = scratch.data_ptr()
    sp += (-sp) % 256                                       # the native layout is 256-byte aligned
    m_flag = torch.empty(2, dtype=torch.int64, device=dev)
    out_keys = torch.empty(n, dtype=torch.int64, device=dev)
    out_vals = torch.empty_like(vals)
    out_count = torch.empty(n, dtype=torch.int32, device=dev)
    check(lib.mp4x_hash_reduce_by_key(int(dtype_of_torch(vals.dtype)), int(op), keys.data_ptr(), n, vals.data_ptr(),
                                      dim, sp, sb, out_keys.data_ptr(), out_vals.data_ptr(),
                                      out_count.data_ptr(), m_flag.data_ptr(), stream_ptr(stream)),
          "mp4x_hash_reduce_by_key")
    m = int(m_flag[0].item())
    return out_keys[:m], out_vals[:m], out_count[:m]


def hash_reduce_by_key_canonical(keys: torch.Tensor, vals: torch.Tensor, op: int, stream=None):
    """K5c (csrc/kernels/sparse_hash.hip): the hash reduce-by-key whose result is a function of its
    input alone — (unique_keys, reduced_rows, counts) in CANONICAL TABLE order: the occupied slots,
    in slot order, of the table that plain linear probing builds from the distinct keys in
    ascending unsigned order (``table_slots(n)`` slots, splitmix64 homes; the definition in torch:
    :func:`mp4x.parallel.sparse.canonical_rbk_torch`), then the run of rows keyed -1, if any.
    Every key's rows combine in input order whatever their number: the values and counts of
    :func:`reduce_by_key`, bit for bit.  The same (dtype, op) pairs as :func:`hash_reduce_by_key`.

    The kernels bound every loop; should a lane pass a bound (it cannot with a sound table), the
    call falls back to :func:`reduce_by_key` and the keys come back ASCENDING instead."""
    _dev_check(keys, vals)
    n = keys.numel()
    if keys.dtype != torch.int64 or vals.dim() not in (1, 2) or vals.shape[0] != n:
        raise ValueError("hash_reduce_by_key_canonical: int64 keys[n] and vals[n] / vals[n, dim]")
    if not hash_rbk_supported(vals.dtype, op):
        raise ValueError(f"hash_reduce_by_key_canonical: {vals.dtype} op {op} not supported")
    dev = keys.device
    dim = 1 if vals.dim() == 1 else int(vals.shape[1])
    keys, vals = keys.contiguous(), vals.contiguous()
    lib = native.hip()
    sb = lib.mp4x_hash_rbk_canonical_scratch_bytes(n)
    scratch = torch.empty(sb + 256, dtype=torch.uint8, device=dev)
    sp = scratch.data_ptr()
    sp += (-sp) % 256                                       # the native layout is 256-byte aligned
    m_flag = torch.empty(2, dtype=torch.int64, device=dev)
    out_keys = torch.empty(n, dtype=torch.int64, device=dev)
    out_vals = torch.empty_like(vals)
    out_count = torch.empty(n, dtype=torch.int32, device=dev)
    check(lib.mp4x_hash_reduce_by_key_canonical(int(dtype_of_torch(vals.dtype)), int(op), keys.data_ptr(), n,
                                                vals.data_ptr(), dim, sp, sb, out_keys.data_ptr(),
                                                out_vals.data_ptr(), out_count.data_ptr(), m_flag.data_ptr(),
                                                stream_ptr(stream)), "mp4x_hash_reduce_by_key_canonical")
    m, bad = m_flag.tolist()                                # one sync for both
    if bad:
        return reduce_by_key(keys, vals, int(op), stream=stream)
    return out_keys[:m], out_vals[:m], out_count[:m]


def dense_reduce_by_key(keys: torch.Tensor, vals: Optional[torch.Tensor], op: int, base: int, stride: int, T: int,
                        stream=None):
    """K5d (csrc/kernels/sparse_hash.hip): reduce-by-key of DENSE keys — ``k // stride - base`` in
    [0, T) — by direct addressing: (unique_keys ascending, reduced_rows, counts), the same as
    :func:`reduce_by_key` bit for bit and in the same order, with no sort.  None when the keys
    were not dense after all (a key outside the table, two keys on one slot): use
    :func:`reduce_by_key`."""
    _dev_check(keys, vals)
    n = keys.numel()
    if keys.dtype != torch.int64 or (vals is not None and (vals.dim() not in (1, 2) or vals.shape[0] != n)):
        raise ValueError("dense_reduce_by_key: int64 keys[n] and vals[n] / vals[n, dim] (or None)")
    if n == 0 or T < 1 or stride < 1 or base < 0 or (vals is not None and not hash_rbk_supported(vals.dtype, op)):
        return None
    dev = keys.device
    dim = 0 if vals is None else (1 if vals.dim() == 1 else int(vals.shape[1]))
    lib = native.hip()
    sb = lib.mp4x_dense_rbk_scratch_bytes(n, T)
    scratch = torch.empty(sb + 256, dtype=torch.uint8, device=dev)
    sp = scratch.data_ptr()
    sp += (-sp) % 256
    m_flag = torch.empty(2, dtype=torch.int64, device=dev)
    out_keys = torch.empty(n, dtype=torch.int64, device=dev)
    out_vals = torch.empty_like(vals) if vals is not None else None
    out_count = torch.empty(n, dtype=torch.int32, device=dev)
    check(lib.mp4x_dense_reduce_by_key(int(dtype_of_torch(vals.dtype)) if vals is not None else 0, int(op),
                                       keys.data_ptr(), n, vals.data_ptr() if vals is not None else None, dim,
                                       int(base), int(stride), int(T), sp, sb, out_keys.data_ptr(),
                                       out_vals.data_ptr() if vals is not None else None, out_count.data_ptr(),
                                       m_flag.data_ptr(), stream_ptr(stream)), "mp4x_dense_reduce_by_key")
    m, bad = m_flag.tolist()                                # one sync for both
    if bad:
        return None
    return out_keys[:m], (out_vals[:m] if out_vals is not None else None), out_count[:m]


def reduce_by_key(keys: torch.Tensor, vals: Optional[torch.Tensor], op: int, key_bits: Optional[int] = None,
                  stream=None):
    """Deterministic reduce-by-key: returns (unique_keys, reduced_vals, counts), keys ascending.

    Rows with equal keys are combined in their input order (stable sort), so inputs laid out
    rank after rank reduce in rank order.  ``key_bits``: the caller guarantees every key is in
    [0, 2**key_bits) (dense dictionary ids), so the radix sort runs over those bits only
    (8 bits per onesweep pass: 3 passes for 2**21 keys instead of 8 for full int64 keys).
    """
    _dev_check(keys, vals)
    n = keys.numel()
    dev = keys.device
    if n == 0:
        d = vals.shape[1] if vals is not None and vals.dim() == 2 else 1
        ev = None if vals is None else torch.empty((0, d) if vals.dim() == 2 else (0,), dtype=vals.dtype, device=dev)
        return keys.new_empty(0), ev, torch.empty(0, dtype=torch.int32, device=dev)
    if key_bits is not None and not 1 <= int(key_bits) <= 63:
        raise ValueError(f"reduce_by_key: key_bits {key_bits} outside [1, 63]")
    sk, perm = sort_pairs(keys, end_bit=key_bits, stream=stream)
    starts, nruns = run_starts(sk, stream=stream)
    dim = 1 if vals is None or vals.dim() == 1 else int(vals[0].numel())
    out_keys = torch.empty(n, dtype=torch.int64, device=dev)
    out_count = torch.empty(n, dtype=torch.int32, device=dev)
    out_vals = None
    if vals is not None:
        if vals.shape[0] != n:
            raise ValueError("reduce_by_key: vals rows != keys")
        out_vals = torch.empty((n,) + tuple(vals.shape[1:]), dtype=vals.dtype, device=dev)
    dt = dtype_of_torch(vals.dtype) if vals is not None else DType.F32
    check(native.hip().mp4x_segment_reduce_rows(int(dt), int(op), sk.data_ptr(), perm.data_ptr(), starts.data_ptr(),
                                                nruns.data_ptr(), n, n,
                                                vals.data_ptr() if vals is not None else None, dim,
                                                out_keys.data_ptr(),
                                                out_vals.data_ptr() if out_vals is not None else None,
                                                out_count.data_ptr(), stream_ptr(stream)), "mp4x_segment_reduce_rows")
    m = int(nruns.item())
    return out_keys[:m], (out_vals[:m] if out_vals is not None else None), out_count[:m]
