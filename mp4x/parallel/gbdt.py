"""Histogram GBDT in exact fixed point (K16): the definitions in torch (also the CPU form) and the
data-parallel trainer on them.

Gradients and hessians are quantised once a tree to int32 with a shift both sides agree on
(:func:`gbdt_shift` of the job-wide largest magnitude), histograms are int64 sums of them and the
split search reads integer prefix sums.  Integer sums do not depend on their order, so a histogram has
the same bits for every block schedule, tile size, rank count and device, the allreduce over ranks is
an exact int64 SUM, and :func:`train_gbdt_quantized` grows bit-identical trees on 1 or p ranks, on the
CPU or the GPU.  Every ``*_torch`` function is the definition; on GPU tensors it runs the HIP kernels
of csrc/kernels/gbdt.hip through :mod:`mp4x.ops.device_ops` (a missing kernel is an error, there is no
torch fallback on the GPU).
"""
from __future__ import annotations

import math
from typing import List

import torch

from ..models.gbdt import Tree
from ..operands import Operands
from ..operators import Operators
from ..ops.device_ops import GbdtSplit

QMAX = 2 ** 31 - 1
MAX_SHIFT = 200
MIN_GAIN = 1e-12


def gbdt_shift(maxabs: float) -> int:
    """The shift s of a tree: with ``maxabs = m * 2**e`` (frexp, m in [0.5, 1)), ``s = 30 - e``, so the
    largest magnitude lands in [2**29, 2**30); 0 for ``maxabs == 0`` or a non-finite one.  Kept inside
    ``+-200``, where ``float64(x) * 2**s`` is exact for every float32 x."""
    maxabs = float(maxabs)
    if maxabs == 0.0 or not math.isfinite(maxabs):
        return 0
    return max(-MAX_SHIFT, min(MAX_SHIFT, 30 - math.frexp(abs(maxabs))[1]))


def _shifts(*shifts) -> None:
    for s in shifts:
        if isinstance(s, bool) or not isinstance(s, int) or abs(s) > MAX_SHIFT:
            raise ValueError(f"the shift {s!r} is not an int in [-{MAX_SHIFT}, {MAX_SHIFT}]")


def gbdt_quantize_torch(g: torch.Tensor, h: torch.Tensor, sg: int, sh: int) -> torch.Tensor:
    """``gh`` int32 ``[n, 2]``: ``q = rint(float64(x) * 2**s)``, half to even (the product only changes
    the exponent, so this is the one rounding), NaN -> 0, clamped to ``+-(2**31 - 1)``."""
    _shifts(sg, sh)
    if g.dtype != torch.float32 or h.dtype != torch.float32 or g.dim() != 1 or h.shape != g.shape:
        raise ValueError("g and h must be float32 [n]")
    if g.is_cuda:
        from ..ops import device_ops
        return device_ops.gbdt_quantize(g.contiguous(), h.contiguous(), sg, sh)

    def q(x, s):
        v = torch.round(x.to(torch.float64) * (2.0 ** s))
        return torch.nan_to_num(v, nan=0.0, posinf=float(QMAX), neginf=-float(QMAX)).clamp_(-QMAX, QMAX).to(torch.int32)
    return torch.stack([q(g, sg), q(h, sh)], dim=1)


def _clamped_bounds(seg: torch.Tensor, m: int) -> List[int]:
    c = [0]
    for hi in seg.tolist()[1:]:
        c.append(max(c[-1], min(int(hi), m)))
    return c


def gbdt_hist_torch(bins: torch.Tensor, gh: torch.Tensor, rows: torch.Tensor, seg: torch.Tensor, B: int) -> torch.Tensor:
    """``hist`` int64 ``[k, F, B, 2]``: ``hist[j, f, b] = sum gh[r]`` over ``r in rows[c[j]:c[j+1]]`` with
    ``bins[r, f] == b``; ``c[0] = 0``, ``c[j+1] = max(c[j], min(seg[j+1], m))`` (any table is legal), a
    row index outside ``[0, n)`` and a bin value ``>= B`` (a missing value) are skipped.  The CPU form
    reads the table on the host; the kernel does not."""
    if isinstance(B, bool) or not isinstance(B, int) or not 2 <= B <= 256:
        raise ValueError(f"B {B!r} must be an int in [2, 256]")
    if bins.dtype != torch.uint8 or bins.dim() != 2 or gh.dtype != torch.int32 or tuple(gh.shape) != (bins.shape[0], 2):
        raise ValueError("bins must be uint8 [n, F] and gh int32 [n, 2]")
    if rows.dtype != torch.int32 or rows.dim() != 1 or seg.dtype != torch.int64 or seg.dim() != 1 or seg.numel() < 1:
        raise ValueError("rows must be int32 [m] and seg int64 [k + 1]")
    if bins.is_cuda:
        from ..ops import device_ops
        return device_ops.gbdt_histogram(bins.contiguous(), gh.contiguous(), rows.contiguous(), seg.contiguous(), B)
    n, F = bins.shape
    m, k = rows.numel(), seg.numel() - 1
    c = _clamped_bounds(seg, m)
    node = torch.repeat_interleave(torch.arange(k), torch.tensor([c[j + 1] - c[j] for j in range(k)], dtype=torch.int64))
    r = rows[:c[k]].to(torch.int64)
    ok = (r >= 0) & (r < n)
    r, node = r[ok], node[ok]
    b = bins[r].to(torch.int64)                                                   # [rows, F]
    cell = (node[:, None] * F + torch.arange(F)[None, :]) * B + b
    live = b < B
    val = gh[r].to(torch.int64)[:, None, :].expand(-1, F, -1)
    hist = torch.zeros(k * F * B, 2, dtype=torch.int64)
    hist.index_add_(0, cell[live], val[live])
    return hist.view(k, F, B, 2)


def gbdt_split_torch(hist: torch.Tensor, sg: int, sh: int, lam: float) -> GbdtSplit:
    """The best split of every node.  Per feature the inclusive int64 prefix sums ``GL, HL`` over the
    bins, ``G, H`` the feature's own last prefix, ``GR = G - GL`` and ``HR = H - HL`` in int64; in float64
    with ``x = int * 2**-s``::

        gain(f, t) = GL*GL / (HL + lam) + GR*GR / (HR + lam) - G*G / (H + lam)      t in [0, B - 2]

    in exactly that order, every operation rounded once.  The largest finite gain wins, ties to the
    lower f, then the lower t; a NaN or infinite gain never wins.  ``gain`` is the winner's (-inf
    without a finite gain); a node whose gain is ``<= 1e-12`` or not finite reports feature -1,
    threshold -1 and ``GL = HL = 0``.  ``G, H`` are the winning feature's, feature 0's without one."""
    _shifts(sg, sh)
    if hist.dtype != torch.int64 or hist.dim() != 4 or hist.shape[3] != 2 or hist.shape[1] < 1 or hist.shape[2] < 2:
        raise ValueError("hist must be int64 [k, F, B, 2] with F >= 1 and B >= 2")
    if hist.is_cuda:
        from ..ops import device_ops
        return device_ops.gbdt_best_split(hist.contiguous(), sg, sh, lam)
    k, F, B, _ = hist.shape
    pre = torch.cumsum(hist, dim=2)
    GLi, HLi = pre[:, :, :-1, 0], pre[:, :, :-1, 1]                               # [k, F, B - 1]
    Gi, Hi = pre[:, :, -1:, 0], pre[:, :, -1:, 1]
    kg, kh, lam = 2.0 ** -sg, 2.0 ** -sh, float(lam)
    gl, hl = GLi.double() * kg, HLi.double() * kh
    gr, hr = (Gi - GLi).double() * kg, (Hi - HLi).double() * kh
    gt, ht = Gi.double() * kg, Hi.double() * kh
    gain = (gl * gl) / (hl + lam) + (gr * gr) / (hr + lam) - (gt * gt) / (ht + lam)
    flat = torch.where(torch.isfinite(gain), gain, torch.full_like(gain, -math.inf)).reshape(k, F * (B - 1))
    best = flat.max(dim=1).values if k else flat.new_zeros(0)
    idx = torch.where(flat == best[:, None], torch.arange(F * (B - 1))[None, :], F * (B - 1)).min(dim=1).values \
        if k else torch.zeros(0, dtype=torch.int64)
    split = torch.isfinite(best) & (best > MIN_GAIN)
    f = torch.where(split, idx // (B - 1), torch.zeros_like(idx))
    t = idx % (B - 1)
    won_gain = flat.gather(1, idx[:, None])[:, 0]                                 # the winner's own bits (+-0)
    rows = torch.arange(k)
    zero = torch.zeros(k, dtype=torch.int64)
    return GbdtSplit(won_gain, torch.where(split, f, -1).to(torch.int32), torch.where(split, t, -1).to(torch.int32),
                     torch.where(split, GLi[rows, f, t], zero), torch.where(split, HLi[rows, f, t], zero),
                     Gi[rows, f, 0], Hi[rows, f, 0])


# ---------------------------------------------------------------- the trainer
def _allreduce(comm, t: torch.Tensor, operand, operator) -> torch.Tensor:
    """In-place allreduce of a flat tensor over the job: the device engine for a GPU tensor, the host
    data plane for a CPU one."""
    if comm is None or comm.getSlaveNum() == 1:
        return t
    if t.is_cuda:
        comm.device.allreduce(t, 0, t.numel(), operator, operand)
    else:
        arr = t.numpy()
        comm.allreduceArray(arr, operand, operator, 0, arr.size)
    return t


def gbdt_level_rows(node_of: torch.Tensor, slot_of_node: torch.Tensor, k: int):
    """``(rows, seg)`` of a level: the rows whose node has a slot, grouped by slot in ascending row
    order (torch's stable sort: K9's count / scatter halves move token rows by an id per assignment and
    return slots, not a row permutation, so they do not serve unchanged), and the int64 ``[k + 1]``
    offsets."""
    slot = slot_of_node[node_of]
    key = torch.where(slot >= 0, slot, torch.full_like(slot, k))
    order = torch.sort(key, stable=True).indices
    counts = torch.bincount(key, minlength=k + 1)[:k]
    seg = torch.zeros(k + 1, dtype=torch.int64, device=node_of.device)
    seg[1:] = torch.cumsum(counts, 0)
    return order.to(torch.int32), seg


def train_gbdt_quantized(comm, bins: torch.Tensor, y: torch.Tensor, B: int, trees: int = 5, depth: int = 3,
                         lr: float = 0.3, lam: float = 1.0) -> List[Tree]:
    """:func:`mp4x.models.gbdt.train_gbdt` on fixed-point statistics: ``bins`` uint8 ``[n, F]`` and ``y``
    ``[n]`` are this rank's rows, torch tensors on the CPU or the GPU.  Squared loss: ``g = float32(pred -
    y)``, ``h = 1``.  Per tree one allreduce MAX of ``(max|g|, max|h|)`` fixes the shifts and the rows are
    quantised once; per level the rows are grouped by node, one histogram call and one int64 SUM allreduce
    give the job's histograms, one split call the ``k`` records the tree grows from on the host, and
    ``node_of`` moves elementwise.  Every step is per row or in integers: the trees are bit for bit the
    same for every rank count and on either device."""
    dev = bins.device
    n, F = bins.shape
    y = y.to(device=dev, dtype=torch.float64)
    pred = torch.zeros(n, dtype=torch.float64, device=dev)
    h = torch.ones(n, dtype=torch.float32, device=dev)
    out: List[Tree] = []
    for _ in range(trees):
        g = (pred - y).to(torch.float32)
        top = torch.stack([g.abs().max() if n else g.new_zeros(()), h.abs().max() if n else h.new_zeros(())]).double()
        top = torch.nan_to_num(top, nan=math.inf)
        top = _allreduce(comm, top, Operands.DOUBLE_OPERAND(), Operators.Double.MAX).tolist()
        sg, sh = gbdt_shift(top[0]), gbdt_shift(top[1])
        gh = gbdt_quantize_torch(g, h, sg, sh)
        node_of = torch.zeros(n, dtype=torch.int64, device=dev)
        tree = Tree([-1], [-1], [-1], [-1], [0.0])
        frontier = [0]
        for level in range(depth + 1):
            k = len(frontier)
            slot_of_node = torch.full((len(tree.value),), -1, dtype=torch.int64)
            slot_of_node[frontier] = torch.arange(k)
            rows, seg = gbdt_level_rows(node_of, slot_of_node.to(dev), k)
            hist = gbdt_hist_torch(bins, gh, rows, seg, B)
            _allreduce(comm, hist.view(-1), Operands.LONG_OPERAND(), Operators.Long.SUM)
            best = gbdt_split_torch(hist, sg, sh, lam)
            rec = [t.tolist() for t in best]
            feat_of = torch.full((len(tree.value),), -1, dtype=torch.int64)
            thr_of = torch.zeros(len(tree.value), dtype=torch.int64)
            left_of = torch.zeros(len(tree.value), dtype=torch.int64)
            new_frontier = []
            for i, nd in enumerate(frontier):
                f, t = rec[1][i], rec[2][i]
                G, H = math.ldexp(rec[5][i], -sg), math.ldexp(rec[6][i], -sh)
                tree.value[nd] = -G / (H + lam) * lr
                if level == depth or H < 2 or f < 0:
                    continue
                li = len(tree.value)
                for _ in range(2):
                    tree.feature.append(-1)
                    tree.threshold.append(-1)
                    tree.left.append(-1)
                    tree.right.append(-1)
                    tree.value.append(0.0)
                tree.feature[nd], tree.threshold[nd], tree.left[nd], tree.right[nd] = f, t, li, li + 1
                feat_of[nd], thr_of[nd], left_of[nd] = f, t, li
                new_frontier += [li, li + 1]
            if not new_frontier:
                break
            feat_of, thr_of, left_of = feat_of.to(dev), thr_of.to(dev), left_of.to(dev)
            f_row = feat_of[node_of]
            moves = f_row >= 0
            b_row = bins.gather(1, f_row.clamp(min=0)[:, None])[:, 0].to(torch.int64)
            child = left_of[node_of] + (b_row > thr_of[node_of]).to(torch.int64)
            node_of = torch.where(moves, child, node_of)
            frontier = new_frontier
        pred += torch.tensor(tree.value, dtype=torch.float64, device=dev)[node_of]
        out.append(tree)
    return out
