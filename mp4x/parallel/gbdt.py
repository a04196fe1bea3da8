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


def gbdt_hist_torch(bins: torch.Tensor, gh: torch.Tensor, rows: torch.Tensor, seg: torch.Tensor, B: int,
                    out: torch.Tensor = None) -> torch.Tensor:
    """``hist`` int64 ``[k, F, B, 2]``: ``hist[j, f, b] = sum gh[r]`` over ``r in rows[c[j]:c[j+1]]`` with
    ``bins[r, f] == b``; ``c[0] = 0``, ``c[j+1] = max(c[j], min(seg[j+1], m))`` (any table is legal), a
    row index outside ``[0, n)`` and a bin value ``>= B`` (a missing value) are skipped.  The CPU form
    reads the table on the host; the kernel does not.  ``out`` receives the result."""
    if isinstance(B, bool) or not isinstance(B, int) or not 2 <= B <= 256:
        raise ValueError(f"B {B!r} must be an int in [2, 256]")
    if bins.dtype != torch.uint8 or bins.dim() != 2 or gh.dtype != torch.int32 or tuple(gh.shape) != (bins.shape[0], 2):
        raise ValueError("bins must be uint8 [n, F] and gh int32 [n, 2]")
    if rows.dtype != torch.int32 or rows.dim() != 1 or seg.dtype != torch.int64 or seg.dim() != 1 or seg.numel() < 1:
        raise ValueError("rows must be int32 [m] and seg int64 [k + 1]")
    if bins.is_cuda:
        from ..ops import device_ops
        return device_ops.gbdt_histogram(bins.contiguous(), gh.contiguous(), rows.contiguous(), seg.contiguous(), B,
                                         out=out)
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
    if out is not None:
        return out.copy_(hist.view(k, F, B, 2))
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


# ---------------------------------------------------------------- the level advance (K17)
def gbdt_partition_torch(bins: torch.Tensor, rows: torch.Tensor, seg: torch.Tensor, feature: torch.Tensor,
                         threshold: torch.Tensor, first_right: torch.Tensor = None, out=None):
    """``(rows2, seg2)``: the stable two-way partition of every segment of a level.  ``seg`` int64 ``[k +
    1]`` is :func:`gbdt_hist_torch`'s table over ``rows`` int32 ``[m]`` (clamped the same way, any table is
    legal), ``feature``, ``threshold``, ``first_right`` int32 ``[k]`` (``first_right`` defaults to 0), ``k <=
    2048``.  Node j splits iff ``0 <= feature[j] < F``; the rows of a node that does not split and a slot
    whose row index is outside ``[0, n)`` are dropped.  Row r of a splitting node goes right iff
    ``int(bins[r, feature[j]]) > threshold[j]`` (any int32 threshold; the trainer's rule, a missing-value
    bin goes right) and is "first" iff ``went_right == (first_right[j] != 0)``, else "second".  ``seg2``
    int64 ``[2k + 1]`` from 0: segment j of ``rows2`` holds node j's first rows, segment ``k + j`` its second
    rows, in slot order, so ``seg2[:k + 1]`` is the table of the first children alone.  Only
    ``rows2[:seg2[2k]]`` is defined: the CPU form fills the rest with -1, the kernels leave it alone.
    ``out=(rows2, seg2)`` receives the result."""
    if bins.dtype != torch.uint8 or bins.dim() != 2 or bins.shape[1] < 1:
        raise ValueError("bins must be uint8 [n, F] with F >= 1")
    if rows.dtype != torch.int32 or rows.dim() != 1 or seg.dtype != torch.int64 or seg.dim() != 1 or seg.numel() < 1:
        raise ValueError("rows must be int32 [m] and seg int64 [k + 1]")
    (n, F), m, k = bins.shape, rows.numel(), seg.numel() - 1
    if first_right is None:
        first_right = torch.zeros(k, dtype=torch.int32, device=bins.device)
    if k > 2048 or any(t.dtype != torch.int32 or tuple(t.shape) != (k,) for t in (feature, threshold, first_right)):
        raise ValueError("feature, threshold and first_right must be int32 [k] with k <= 2048")
    if bins.is_cuda:
        from ..ops import device_ops
        return device_ops.gbdt_partition(bins.contiguous(), rows.contiguous(), seg.contiguous(), feature.contiguous(),
                                         threshold.contiguous(), first_right.contiguous(), out=out)
    c = _clamped_bounds(seg, m)
    node = torch.repeat_interleave(torch.arange(k), torch.tensor([c[j + 1] - c[j] for j in range(k)], dtype=torch.int64))
    r = rows[:c[k]].to(torch.int64)
    f = feature.to(torch.int64)[node]
    live = (r >= 0) & (r < n) & (f >= 0) & (f < F)
    r, f, node = r[live], f[live], node[live]
    right = bins[r, f].to(torch.int64) > threshold.to(torch.int64)[node]
    key = torch.where(right == (first_right[node] != 0), node, node + k)
    rows2 = torch.full((m,), -1, dtype=torch.int32)
    rows2[:r.numel()] = r[torch.sort(key, stable=True).indices].to(torch.int32)
    seg2 = torch.zeros(2 * k + 1, dtype=torch.int64)
    seg2[1:] = torch.cumsum(torch.bincount(key, minlength=2 * k), 0)
    if out is not None:
        out[0].copy_(rows2)
        out[1].copy_(seg2)
        return out[0], out[1]
    return rows2, seg2


def gbdt_hist_subtract_torch(parent: torch.Tensor, small: torch.Tensor, parent_of: torch.Tensor,
                             out: torch.Tensor = None) -> torch.Tensor:
    """Sibling subtraction: ``large[p] = parent[parent_of[p]] - small[p]`` in wrapping int64, ``parent``
    int64 ``[k, F, B, 2]``, ``small`` int64 ``[kp, F, B, 2]``, ``parent_of`` int32 ``[kp]``; a ``parent_of[p]``
    outside ``[0, k)`` reads a zero histogram.  Histograms are exact integer sums, so this is the other
    child's histogram bit for bit."""
    if parent.dtype != torch.int64 or parent.dim() != 4 or parent.shape[3] != 2 or small.dtype != torch.int64 or \
            small.dim() != 4 or small.shape[1:] != parent.shape[1:] or parent_of.dtype != torch.int32 or \
            tuple(parent_of.shape) != (small.shape[0],):
        raise ValueError("parent must be int64 [k, F, B, 2], small int64 [kp, F, B, 2] and parent_of int32 [kp]")
    if parent.is_cuda:
        from ..ops import device_ops
        return device_ops.gbdt_hist_subtract(parent.contiguous(), small.contiguous(), parent_of.contiguous(), out=out)
    k = parent.shape[0]
    j = parent_of.to(torch.int64)
    inside = (j >= 0) & (j < k)
    zero = torch.zeros((1,) + tuple(parent.shape[1:]), dtype=torch.int64)
    large = torch.cat([parent, zero])[torch.where(inside, j, torch.full_like(j, k))] - small
    if out is not None:
        out.copy_(large)
        return out
    return large


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
                         lr: float = 0.3, lam: float = 1.0, level: str = "sort", subtract: bool = False) -> List[Tree]:
    """:func:`mp4x.models.gbdt.train_gbdt` on fixed-point statistics: ``bins`` uint8 ``[n, F]`` and ``y``
    ``[n]`` are this rank's rows, torch tensors on the CPU or the GPU.  Squared loss: ``g = float32(pred -
    y)``, ``h = 1``.  Per tree one allreduce MAX of ``(max|g|, max|h|)`` fixes the shifts and the rows are
    quantised once; per level the rows are grouped by node, one histogram call and one int64 SUM allreduce
    give the job's histograms, one split call the ``k`` records the tree grows from on the host, and
    ``node_of`` moves elementwise.  Every step is per row or in integers: the trees are bit for bit the
    same for every rank count and on either device.

    ``level`` is how a level's rows are grouped: ``"sort"`` sorts all rows by node
    (:func:`gbdt_level_rows`); ``"partition"`` keeps the rows grouped from level to level and splits every
    segment in two with :func:`gbdt_partition_torch` (K17), two row buffers in turn, the split records
    uploaded per segment and the next table taken from ``seg2`` by device indexing.  ``subtract=True``
    (``level="partition"`` only) puts the child with the smaller hessian mass first (right iff ``H - HL <
    HL`` of the allreduced record: the same on every rank), histograms and allreduces the first children
    alone and takes every sibling as parent - child (:func:`gbdt_hist_subtract_torch`), exactly.  Both
    grow the default's trees bit for bit."""
    if level not in ("sort", "partition"):
        raise ValueError(f"level {level!r} must be 'sort' or 'partition'")
    if subtract and level != "partition":
        raise ValueError("subtract=True needs level='partition'")
    part = level == "partition"
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
        seg_nodes = [0]                                   # partition: the tree node of every segment
        if part:
            rows, spare = torch.arange(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
            seg = torch.tensor([0, n], dtype=torch.int64, device=dev)
        hist, parents = None, []
        for level_no in range(depth + 1):
            k = len(frontier)
            if not part:
                slot_of_node = torch.full((len(tree.value),), -1, dtype=torch.int64)
                slot_of_node[frontier] = torch.arange(k)
                rows, seg = gbdt_level_rows(node_of, slot_of_node.to(dev), k)
            if subtract and parents:
                kp = len(parents)
                both = torch.empty((2 * kp,) + tuple(hist.shape[1:]), dtype=torch.int64, device=dev)
                gbdt_hist_torch(bins, gh, rows, seg[:kp + 1], B, out=both[:kp])
                _allreduce(comm, both[:kp].view(-1), Operands.LONG_OPERAND(), Operators.Long.SUM)
                gbdt_hist_subtract_torch(hist, both[:kp], torch.tensor(parents, dtype=torch.int32, device=dev),
                                         out=both[kp:])
                hist = both
            else:
                hist = gbdt_hist_torch(bins, gh, rows, seg, B)
                _allreduce(comm, hist.view(-1), Operands.LONG_OPERAND(), Operators.Long.SUM)
            best = gbdt_split_torch(hist, sg, sh, lam)
            rec = [t.tolist() for t in best]
            feat_of = torch.full((len(tree.value),), -1, dtype=torch.int64)
            thr_of = torch.zeros(len(tree.value), dtype=torch.int64)
            left_of = torch.zeros(len(tree.value), dtype=torch.int64)
            seg_of = {nd: i for i, nd in enumerate(seg_nodes)} if part else {nd: i for i, nd in enumerate(frontier)}
            new_frontier = []
            for nd in frontier:
                i = seg_of[nd]
                f, t = rec[1][i], rec[2][i]
                G, H = math.ldexp(rec[5][i], -sg), math.ldexp(rec[6][i], -sh)
                tree.value[nd] = -G / (H + lam) * lr
                if level_no == depth or H < 2 or f < 0:
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
            if part:
                # per segment: the split (-1: a final leaf) and which child stands first
                sf = [tree.feature[nd] for nd in seg_nodes]
                fr = [int(subtract and f >= 0 and rec[6][i] - rec[4][i] < rec[4][i]) for i, f in enumerate(sf)]
                up = torch.tensor([sf, [tree.threshold[nd] for nd in seg_nodes], fr], dtype=torch.int32).to(dev)
                seg2 = torch.empty(2 * k + 1, dtype=torch.int64, device=dev)
                gbdt_partition_torch(bins, rows, seg, up[0], up[1], up[2], out=(spare, seg2))
                rows, spare = spare, rows
                parents = [i for i, f in enumerate(sf) if f >= 0]
                seg = seg2[torch.tensor(parents + [k + i for i in parents] + [2 * k]).to(dev)]
                seg_nodes = [tree.left[seg_nodes[i]] + fr[i] for i in parents] + \
                            [tree.left[seg_nodes[i]] + 1 - fr[i] for i in parents]
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
