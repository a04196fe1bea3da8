"""Histogram GBDT in exact fixed point (K16, K17), the forest walk that applies a trained model (K18), the
binning of float features that both start from (K19), the walk over float features that needs no bins
(K20) and the classification losses with their fused gradient ops (K21): the definitions in torch (also the
CPU form) and the data-parallel trainer on them.

Gradients and hessians are quantised once a tree to int32 with a shift both sides agree on
(:func:`gbdt_shift` of the job-wide largest magnitude), histograms are int64 sums of them and the
split search reads integer prefix sums.  Integer sums do not depend on their order, so a histogram has
the same bits for every block schedule, tile size, rank count and device, the allreduce over ranks is
an exact int64 SUM, and :func:`train_gbdt_quantized` grows bit-identical trees on 1 or p ranks, on the
CPU or the GPU.  Every ``*_torch`` function is the definition; on GPU tensors it runs the HIP kernels
of csrc/kernels/gbdt*.hip through :mod:`mp4x.ops.device_ops` (a missing kernel is an error, there is no
torch fallback on the GPU).
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Sequence

import torch

from ..models.gbdt import Tree
from ..operands import Operands
from ..operators import Operators
from ..ops import gbdt_args
from ..ops.device_ops import GbdtSplit
from ..ops.gbdt_args import MAX_SHIFT, MAX_STEPS, QMAX

MIN_GAIN = 1e-12


def gbdt_shift(maxabs: float) -> int:
    """The shift s of a tree: with ``maxabs = m * 2**e`` (frexp, m in [0.5, 1)), ``s = 30 - e``, so the
    largest magnitude lands in [2**29, 2**30); 0 for ``maxabs == 0`` or a non-finite one.  Kept inside
    ``+-200``, where ``float64(x) * 2**s`` is exact for every float32 x."""
    maxabs = float(maxabs)
    if maxabs == 0.0 or not math.isfinite(maxabs):
        return 0
    return max(-MAX_SHIFT, min(MAX_SHIFT, 30 - math.frexp(abs(maxabs))[1]))


def gbdt_quantize_torch(g: torch.Tensor, h: torch.Tensor, sg: int, sh: int) -> torch.Tensor:
    """``gh`` int32 ``[n, 2]``: ``q = rint(float64(x) * 2**s)``, half to even (the product only changes
    the exponent, so this is the one rounding), NaN -> 0, clamped to ``+-(2**31 - 1)``."""
    gbdt_args.quantize(g, h, sg, sh)
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
    n, F, m, k = gbdt_args.histogram(bins, gh, rows, seg, B)
    if bins.is_cuda:
        from ..ops import device_ops
        return device_ops.gbdt_histogram(bins.contiguous(), gh.contiguous(), rows.contiguous(), seg.contiguous(), B,
                                         out=out)
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
    k, F, B = gbdt_args.split(hist, sg, sh)
    if hist.is_cuda:
        from ..ops import device_ops
        return device_ops.gbdt_best_split(hist.contiguous(), sg, sh, lam)
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
    MAX_PARENTS`` (2048).  Node j splits iff ``0 <= feature[j] < F``; the rows of a node that does not split and a slot
    whose row index is outside ``[0, n)`` are dropped.  Row r of a splitting node goes right iff
    ``int(bins[r, feature[j]]) > threshold[j]`` (any int32 threshold; the trainer's rule, a missing-value
    bin goes right) and is "first" iff ``went_right == (first_right[j] != 0)``, else "second".  ``seg2``
    int64 ``[2k + 1]`` from 0: segment j of ``rows2`` holds node j's first rows, segment ``k + j`` its second
    rows, in slot order, so ``seg2[:k + 1]`` is the table of the first children alone.  Only
    ``rows2[:seg2[2k]]`` is defined: the CPU form fills the rest with -1, the kernels leave it alone.
    ``out=(rows2, seg2)`` receives the result."""
    n, F, m, k = gbdt_args.partition(bins, rows, seg, feature, threshold, first_right)
    if first_right is None:
        first_right = torch.zeros(k, dtype=torch.int32, device=bins.device)
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
    k = gbdt_args.subtract(parent, small, parent_of)[0]
    if parent.is_cuda:
        from ..ops import device_ops
        return device_ops.gbdt_hist_subtract(parent.contiguous(), small.contiguous(), parent_of.contiguous(), out=out)
    j = parent_of.to(torch.int64)
    inside = (j >= 0) & (j < k)
    zero = torch.zeros((1,) + tuple(parent.shape[1:]), dtype=torch.int64)
    large = torch.cat([parent, zero])[torch.where(inside, j, torch.full_like(j, k))] - small
    if out is not None:
        out.copy_(large)
        return out
    return large


# ---------------------------------------------------------------- the forest walk (K18)
class GbdtForest(NamedTuple):
    nodes: torch.Tensor       # int32 [N, 4]: (feature, threshold, left, right), children relative to the tree's first
    #                           node; a leaf has feature -1
    value: torch.Tensor       # float64 [N]: the exact bits of Tree.value, inner nodes too
    tree_off: torch.Tensor    # int32 [T + 1] from 0
    steps: int                # the longest root-to-leaf path of the forest, in edges


def _tree_depth(tree: Tree, t: int) -> int:
    """The longest path below node 0 in edges; ValueError for a child outside the tree or a cycle."""
    size = len(tree.value)
    kids = []
    for j in range(size):
        if tree.left[j] < 0:
            kids.append(())
            continue
        if not (0 <= tree.left[j] < size and 0 <= tree.right[j] < size and tree.feature[j] >= 0):
            raise ValueError(f"tree {t}: node {j} has a child outside the tree's {size} nodes or no feature")
        kids.append((tree.left[j], tree.right[j]))
    depth = [-1] * size                                     # -1: not seen, -2: on the path being walked
    stack = [0] if size else []
    while stack:
        j = stack[-1]
        if depth[j] == -1:
            depth[j] = -2
            for c in kids[j]:
                if depth[c] == -2:
                    raise ValueError(f"tree {t}: a cycle through node {c}")
                if depth[c] == -1:
                    stack.append(c)
        else:
            stack.pop()
            if depth[j] == -2:
                depth[j] = 1 + max(depth[c] for c in kids[j]) if kids[j] else 0
    return depth[0] if size else 0


def pack_forest(trees: Sequence[Tree], device=None) -> GbdtForest:
    """The trees as the tensors :func:`gbdt_predict_torch` walks, on ``device``.  A node of a
    :class:`~mp4x.models.gbdt.Tree` is inner iff ``left >= 0``; ValueError for an inner node with a child
    outside its tree or without a feature, for a cycle and for a path longer than ``MAX_STEPS`` edges."""
    rows, value, off, steps = [], [], [0], 0
    for t, tree in enumerate(trees):
        steps = max(steps, _tree_depth(tree, t))
        if steps > MAX_STEPS:
            raise ValueError(f"tree {t}: a path of {steps} edges, at most {MAX_STEPS}")
        for j in range(len(tree.value)):
            inner = tree.left[j] >= 0
            rows.append((tree.feature[j] if inner else -1, tree.threshold[j], tree.left[j], tree.right[j]))
        value += tree.value
        off.append(len(value))
    if len(value) >= 2 ** 31:
        raise ValueError("a forest holds fewer than 2**31 nodes")
    return GbdtForest(torch.tensor(rows, dtype=torch.int32).reshape(-1, 4).to(device),
                      torch.tensor(value, dtype=torch.float64).to(device), torch.tensor(off, dtype=torch.int32).to(device),
                      steps)


def gbdt_predict_torch(bins: torch.Tensor, forest: GbdtForest, init: Optional[torch.Tensor] = None, leaves: bool = False,
                       out=None):
    """``pred`` float64 ``[n]``, and ``leaf`` int32 ``[n, T]`` with ``leaves``: the forest applied to the rows of
    ``bins`` uint8 ``[n, F]``.  The tensors of ``forest`` may hold any bits.  Tree t owns the nodes ``[o[t], o[t +
    1])`` with ``o[0] = 0`` and ``o[t + 1] = max(o[t], min(tree_off[t + 1], N))``, ``size_t`` of them.  The walk of a
    row in tree t starts at node 0 and takes exactly ``forest.steps`` steps.  Node j is inner iff ``0 <= feature <
    F``, ``0 <= left < size_t`` and ``0 <= right < size_t``; there the row moves to ``right`` iff ``int(bins[r,
    feature]) > threshold`` (any int32 threshold; the trainer's rule, a missing-value bin goes right), else to
    ``left``; at any other node it stays.  ``pred[r]`` starts as ``init[r]`` (float64 ``[n]``) or ``+0.0``; the trees
    are taken in ascending order and a tree with nodes adds ``value[o[t] + j]``, one float64 addition, and gives
    ``leaf[r, t] = j``; a tree without nodes adds nothing and gives -1.  ``T = 0`` returns ``init`` bit for bit.
    The order of the sum is fixed, so this form, the kernel and ``sum(tree.predict_bins(...))`` in tree order
    agree bit for bit.  ``out`` receives ``pred`` (the pair ``(pred, leaf)`` with ``leaves``); ``pred`` may be
    ``init``."""
    gbdt_args.predict(bins, forest.nodes, forest.value, forest.tree_off, forest.steps, init)
    if bins.is_cuda:
        from ..ops import device_ops
        return device_ops.gbdt_predict(bins.contiguous(), forest.nodes.contiguous(), forest.value.contiguous(),
                                       forest.tree_off.contiguous(), forest.steps,
                                       None if init is None else init.contiguous(), leaves=leaves, out=out)
    return _walk_torch(bins, forest.nodes[:, 1].to(torch.int64), forest, init, leaves, out)


def _walk_torch(cols: torch.Tensor, thr_of: torch.Tensor, forest: GbdtForest, init, leaves: bool, out):
    """The walk both definitions share, on the CPU: ``cols`` ``[n, F]`` holds integers, ``thr_of`` int64 ``[N]``, and at
    an inner node a row moves right iff ``int(cols[r, feature]) > thr_of[node]``."""
    (n, F), T, N = cols.shape, forest.tree_off.numel() - 1, forest.value.numel()
    o = _clamped_bounds(forest.tree_off, N)
    pred = torch.zeros(n, dtype=torch.float64) if init is None else init.clone()
    leaf = torch.full((n, T), -1, dtype=torch.int32)
    for t in range(T):
        size = o[t + 1] - o[t]
        if size == 0:
            continue
        f, _, left, right = forest.nodes[o[t]:o[t + 1]].to(torch.int64).unbind(1)
        thr = thr_of[o[t]:o[t + 1]]
        inner = (f >= 0) & (f < F) & (left >= 0) & (left < size) & (right >= 0) & (right < size)
        j = torch.zeros(n, dtype=torch.int64)
        for _ in range(forest.steps):
            b = cols.gather(1, torch.where(inner, f, torch.zeros_like(f))[j][:, None])[:, 0].to(torch.int64)
            j = torch.where(inner[j], torch.where(b > thr[j], right[j], left[j]), j)
        pred = pred + forest.value[o[t]:o[t + 1]][j]
        leaf[:, t] = j.to(torch.int32)
    if out is not None:
        outs = tuple(out) if leaves else (out,)
        outs[0].copy_(pred)
        if leaves:
            outs[1].copy_(leaf)
        return outs if leaves else outs[0]
    return (pred, leaf) if leaves else pred


def predict_gbdt(trees: Sequence[Tree], bins: torch.Tensor, init: Optional[torch.Tensor] = None,
                 edges=None, classes: Optional[int] = None) -> torch.Tensor:
    """The sum of the trees' predictions for the rows of ``bins`` uint8 ``[n, F]``, on the device of ``bins``.  With
    ``edges=(edges, cnt)``, those the bins of the training rows were made with, ``bins`` is instead the float features
    ``X`` ``[n, F]`` themselves: the thresholds become keys (:func:`float_forest`) and the rows are walked as they are
    (:func:`gbdt_predict_float_torch`), which gives what binning them first would, bit for bit.  With ``classes=C``
    the trees are round-major as ``train_gbdt_quantized(loss="softmax")`` returns them and the result is the
    margins float64 ``[C, n]``: class c is this call over ``trees[c::C]`` (``init`` float64 ``[C, n]``)."""
    if classes is not None:
        if isinstance(classes, bool) or not isinstance(classes, int) or classes < 1 or len(trees) % classes:
            raise ValueError(f"classes {classes!r} must be an int >= 1 that divides the {len(trees)} trees")
        return torch.stack([predict_gbdt(trees[c::classes], bins, None if init is None else init[c], edges)
                            for c in range(classes)])
    forest = pack_forest(trees, bins.device)
    if edges is None:
        return gbdt_predict_torch(bins, forest, init=init)
    e, c = edges
    return gbdt_predict_float_torch(bins, float_forest(forest, e.to(bins.device), c.to(bins.device)), init=init)


# ---------------------------------------------------------------- the forest walk over float features (K20)
_NAN_KEY = 0xfffffffe                 # kNanKey (gbdt_fwalk_map.hpp): the key of a NaN row, above every other row's
_NEVER = 0xffffffff


def _ukeys(x: torch.Tensor) -> torch.Tensor:
    """``key`` of csrc/kernels/gbdt_bin_map.hpp for float32 values, as int64 in ``[0, 2**32)``: unsigned order is the
    IEEE order of the non-NaN values, ``-0.0`` takes the key of ``+0.0``; a NaN takes ``_NAN_KEY``.  Bit operations
    only."""
    u = x.contiguous().view(torch.int32).to(torch.int64) & 0xffffffff
    u = torch.where(u == 0x80000000, torch.zeros_like(u), u)
    k = torch.where(u >= 0x80000000, u ^ 0xffffffff, u | 0x80000000)
    return torch.where((u & 0x7fffffff) > 0x7f800000, torch.full_like(u, _NAN_KEY), k)


def float_forest(forest: GbdtForest, edges: torch.Tensor, cnt: torch.Tensor) -> GbdtForest:
    """``forest`` with every bin threshold replaced by a uint32 key ``K`` (kept as its int32 bits) that
    :func:`gbdt_predict_float_torch` compares the keys of float features with: for rows binned by
    :func:`gbdt_bin_torch` under ``edges`` float32 ``[F, E]`` and ``cnt`` int32 ``[F]`` with ``missing = 255``, the walk of
    the float rows through the result ends where the walk of their bins through ``forest`` does.  With ``f, t`` a
    node's feature and threshold and ``c = clamp(cnt[f], 0, E)``::

        t < 0          K = 0                      everyone goes right
        0 <= t < c     K = key(edges[f, t])       NaN rows, and rows with edges[f, t] <= x
        c <= t < 255   K = 0xfffffffe             only a NaN row (its bin is 255)
        t >= 255       K = 0xffffffff             nobody
        f outside [0, F)   K = 0xffffffff         (the node is never inner)

    For non-decreasing non-NaN edges a row's bin is the number of ``e < c`` with ``edges[f, e] <= x``, so ``bin > t``
    iff ``t < 0`` or (``t < c`` and ``edges[f, t] <= x``); ValueError if ``edges[f, :c]`` of a feature some node names
    holds a NaN or descends (:func:`gbdt_edges` gives neither).  ``value``, ``tree_off`` and ``steps`` are the
    forest's own.  Torch on the forest's device, once a model."""
    F, E = gbdt_args.float_forest(forest.nodes, edges, cnt)
    f, t = forest.nodes[:, 0].to(torch.int64), forest.nodes[:, 1].to(torch.int64)
    named = (f >= 0) & (f < F)
    c_of = cnt.clamp(0, E).to(torch.int64)
    used = torch.zeros(F, dtype=torch.bool, device=edges.device)
    used[f[named]] = True
    inside = (torch.arange(E, device=edges.device)[None, :] < c_of[:, None]) & used[:, None]
    if bool((edges.isnan() & inside).any()) or bool(((edges[:, 1:] < edges[:, :-1]) & inside[:, 1:]).any()):
        raise ValueError("edges[f, :cnt[f]] of a feature the forest names holds a NaN or is not non-decreasing")
    fc = f.clamp(0, F - 1)
    c = c_of[fc]
    edge_key = _ukeys(edges[fc, t.clamp(0, E - 1)]) if E else torch.zeros_like(t)
    K = torch.where(t < 0, torch.zeros_like(t), torch.where(
        t < c, edge_key, torch.where(t < 255, torch.full_like(t, _NAN_KEY), torch.full_like(t, _NEVER))))
    K = torch.where(named, K, torch.full_like(K, _NEVER))
    nodes = forest.nodes.clone()
    nodes[:, 1] = torch.where(K >= 2 ** 31, K - 2 ** 32, K).to(torch.int32)
    return GbdtForest(nodes, forest.value, forest.tree_off, forest.steps)


def gbdt_predict_float_torch(X: torch.Tensor, fforest: GbdtForest, init: Optional[torch.Tensor] = None,
                             leaves: bool = False, out=None):
    """:func:`gbdt_predict_torch` over the float features ``X`` ``[n, F]`` (float32, or float16 / bfloat16 widened to
    float32, which is exact; contiguous on the GPU) and a forest of :func:`float_forest`: the same tree table,
    ``is_inner`` rule, ``steps`` steps, float64 sums in tree order, ``init``, ``out`` and ``leaves``.  The one change is
    the step: with ``K`` the node's second field read as uint32 and ``xkey`` the key of ``X[r, feature]`` (``key`` of
    csrc/kernels/gbdt_bin_map.hpp for a non-NaN value, ``0xfffffffe`` for a NaN), the row moves right iff ``K <=
    xkey``.  Any bits are legal in the forest and in ``X``.  One launch on the GPU and no bin tensor."""
    gbdt_args.predict_float(X, fforest.nodes, fforest.value, fforest.tree_off, fforest.steps, init)
    if X.is_cuda:
        from ..ops import device_ops
        return device_ops.gbdt_predict_float(X, fforest.nodes.contiguous(), fforest.value.contiguous(),
                                             fforest.tree_off.contiguous(), fforest.steps,
                                             None if init is None else init.contiguous(), leaves=leaves, out=out)
    # K <= xkey iff xkey > K - 1 in integers
    return _walk_torch(_ukeys(X.to(torch.float32)), (fforest.nodes[:, 1].to(torch.int64) & 0xffffffff) - 1, fforest,
                       init, leaves, out)


# ---------------------------------------------------------------- feature binning (K19)
_SEARCH_STEPS = (128, 64, 32, 16, 8, 4, 2, 1)
_SORT_CHUNK = 1 << 24                 # elements one torch.sort call takes: bounds its int64 index tensor


def gbdt_bin_torch(X: torch.Tensor, edges: torch.Tensor, cnt: torch.Tensor, missing: int = 255,
                   out: torch.Tensor = None) -> torch.Tensor:
    """``bins`` uint8 ``[n, F]`` of the features ``X`` ``[n, F]`` (float32, or float16 / bfloat16 widened to float32,
    which is exact; contiguous on the GPU) under ``edges`` float32 ``[F, E]``, ``E <= MAX_EDGES`` (255), and ``cnt``
    int32 ``[F]``.  The tensors may hold any bits.  With ``c = clamp(cnt[f], 0, E)`` and ``x = X[r, f]``::

        pos = 0
        for s in (128, 64, 32, 16, 8, 4, 2, 1):
            if pos + s <= c and edges[f, pos + s - 1] <= x:
                pos += s
        bin = missing if x is NaN else pos

    The compare is float32 IEEE: denormals are not flushed, ``-0.0 == +0.0``, a NaN edge is never ``<= x``, ``+-inf``
    are ordinary values.  This fixed search is the definition, so unsorted or NaN edges have one answer too; for
    ascending edges it is ``searchsorted(edges[f, :c], x, side="right")``, the rule of
    :func:`mp4x.models.gbdt.quantize`.  ``pos <= c <= 255``.  A NaN lands in ``missing`` (an int in ``[0, 255]``): with
    ``B <= 255`` bins and ``missing = 255`` the histogram skips it and the partition and the walk send it right, as
    K16-K18 define for a bin ``>= B``; with ``B = 256`` bin 255 is an ordinary bin, shared with the largest
    values.  ``out`` receives the result."""
    n, F, E = gbdt_args.bin(X, edges, cnt, missing)
    if X.is_cuda:
        from ..ops import device_ops
        return device_ops.gbdt_bin(X, edges.contiguous(), cnt.contiguous(), missing, out=out)
    x = X.to(torch.float32)
    c = cnt.clamp(0, E).to(torch.int64)[None, :]
    pos = torch.zeros(n, F, dtype=torch.int64)
    by_entry = edges.t()                                                          # [E, F]
    for s in _SEARCH_STEPS if E else ():
        entry = by_entry.gather(0, (pos + s - 1).clamp(max=E - 1))
        pos = torch.where((pos + s <= c) & (entry <= x), pos + s, pos)
    bins = torch.where(torch.isnan(x), torch.full_like(pos, missing), pos).to(torch.uint8)
    if out is not None:
        return out.copy_(bins)
    return bins


def _float_keys(X: torch.Tensor) -> torch.Tensor:
    """int32 keys of the values widened to float32 whose signed order is the order of the floats: ``-0.0`` takes
    the key of ``+0.0``, a NaN the largest int32, which is the key of no other value (``+inf``'s is below it).  Bit
    operations only, so both devices give the same keys whatever their float modes."""
    u = X.to(torch.float32).view(torch.int32)
    u = torch.where(u == -2 ** 31, torch.zeros_like(u), u)
    nan = (u & 0x7fffffff) > 0x7f800000
    return torch.where(nan, torch.full_like(u, 2 ** 31 - 1), torch.where(u < 0, u ^ 0x7fffffff, u))


def _key_floats(k: torch.Tensor) -> torch.Tensor:
    """The float32 values of :func:`_float_keys`' keys (int32; none of them a NaN's)."""
    return torch.where(k < 0, k ^ 0x7fffffff, k).view(torch.float32)


def gbdt_edges(comm, X: torch.Tensor, B: int):
    """``(edges float32 [F, B - 1], cnt int32 [F])``: exact quantile edges of the job's rows, the same bits for
    every sharding of the rows over the ranks and on either device.  ``X`` ``[n, F]`` (float32, float16 or
    bfloat16) are this rank's rows, ``2 <= B <= 256``.  Per feature, the job-wide multiset of the non-NaN values,
    widened to float32 with ``-0.0`` taken as ``+0.0``, has ``N_f`` members; the candidate ``q = 1 .. B - 1`` is its
    order statistic of 0-based rank ``(q * N_f) // B`` (integers, no interpolation: an input value).
    ``edges[f, :cnt[f]]`` are the distinct candidates ascending, the rest of the row is ``+inf``; ``N_f = 0`` gives
    ``cnt[f] = 0``.

    Every rank sorts its own columns once (order-preserving int32 keys, ``torch.sort`` in feature chunks); one
    int64 SUM allreduce gives ``N_f``; then 32 rounds of bisection on the key find all ``F * (B - 1)`` order
    statistics at once, each round one batched ``searchsorted`` on the local columns and one int64 SUM
    allreduce of the ``[F, B - 1]`` counts: the wanted key is the smallest ``K`` with ``count(keys <= K) >= rank +
    1``.  Only integer counts cross ranks, so the sharding cannot show."""
    n, F = gbdt_args.edges(X, B)
    dev, E = X.device, B - 1
    long_sum = (Operands.LONG_OPERAND(), Operators.Long.SUM)
    per_call = max(1, _SORT_CHUNK // max(n, 1))
    cols = torch.cat([torch.sort(_float_keys(X[:, f:f + per_call]).t().contiguous(), dim=1).values
                      for f in range(0, F, per_call)]) if F else torch.empty(0, n, dtype=torch.int32, device=dev)
    N = _allreduce(comm, (cols != 2 ** 31 - 1).sum(dim=1), *long_sum)             # [F] int64
    rank = torch.arange(1, B, device=dev)[None, :] * N[:, None] // B              # [F, E] int64
    lo = torch.full((F, E), -2 ** 31, dtype=torch.int64, device=dev)
    hi = torch.full((F, E), int(_float_keys(torch.tensor([math.inf]))), dtype=torch.int64, device=dev)
    for _ in range(32):                                                           # hi - lo < 2**32 halves to 0
        mid = (lo + hi) >> 1
        below = torch.searchsorted(cols, mid.to(torch.int32), right=True)         # local keys <= mid; never a NaN's
        below = _allreduce(comm, below.to(torch.int64).view(-1), *long_sum).view(F, E)
        found = below >= rank + 1
        hi = torch.where(found, mid, hi)
        lo = torch.where(found, lo, mid + 1)
    cand = lo.to(torch.int32)                                                     # non-decreasing along q
    first = torch.ones(F, E, dtype=torch.bool, device=dev)
    first[:, 1:] = cand[:, 1:] != cand[:, :-1]
    cnt = torch.where(N > 0, first.sum(dim=1), torch.zeros_like(N))
    front = torch.sort((~first).to(torch.uint8), dim=1, stable=True).indices      # the distinct ones first, in order
    edges = _key_floats(cand.gather(1, front))
    edges = torch.where(torch.arange(E, device=dev)[None, :] < cnt[:, None], edges, torch.full_like(edges, math.inf))
    return edges, cnt.to(torch.int32)


def fit_bins(comm, X: torch.Tensor, B: int, missing: int = 255):
    """``(bins, edges, cnt)``: :func:`gbdt_edges` of the job's rows, then :func:`gbdt_bin_torch` of this rank's, on
    the device of ``X``: what :func:`train_gbdt_quantized` and :func:`predict_gbdt` start from."""
    edges, cnt = gbdt_edges(comm, X, B)
    return gbdt_bin_torch(X, edges, cnt, missing), edges, cnt


# ---------------------------------------------------------------- losses (K21)
_LN2_HI, _LN2_LO = float.fromhex("0x1.62e42fee00000p-1"), float.fromhex("0x1.a39ef35793c76p-33")
_INV_LN2 = float.fromhex("0x1.71547652b82fep+0")
_EXP_C = [1.0 / math.factorial(j) for j in range(14)]      # int / int is rounded once: the nearest float64 of 1 / j!
_CLAMP = 708.0


def _exp_neg(t: torch.Tensor) -> torch.Tensor:
    """``exp_neg`` of csrc/kernels/gbdt_loss_map.hpp, operation for operation: ``exp(-t)`` for float64 ``t`` in ``[0,
    708]``, a NaN staying itself."""
    nan = t.isnan()
    x = -torch.where(nan, torch.zeros_like(t), t)
    k = torch.round(x * _INV_LN2)
    r = (x - k * _LN2_HI) - k * _LN2_LO
    p = torch.full_like(r, _EXP_C[13])
    for c in _EXP_C[12::-1]:
        p = p * r
        p = p + c
    scale = ((k.to(torch.int64) + 1023) << 52).view(torch.float64)
    return torch.where(nan, t, p * scale)


def _clamp_t(t: torch.Tensor) -> torch.Tensor:
    return torch.where(t > _CLAMP, torch.full_like(t, _CLAMP), t)          # a NaN passes


def gbdt_grad_torch(pred: torch.Tensor, y: torch.Tensor, loss: str = "squared"):
    """``(g, h)`` float32 of ``pred``'s shape: the gradient and the hessian of ``loss`` at the margins ``pred``.  The
    definition of K21: every step is one float64 operation rounded once, then one rounding to float32 - no library
    ``exp`` - and csrc/kernels/gbdt_loss_map.hpp is the same steps in C++, so the CPU, the GPU and any rank count
    give the same bits.

    ``"squared"``: ``pred``, ``y`` float64 ``[n]``; ``g = float32(pred - y)``, ``h = 1``.

    ``"logistic"``: the same shapes, ``y`` any float64.  ``e = exp_neg(min(|x|, 708))``, ``d = 1 + e``, ``p = 1 / d`` if
    ``x >= 0`` else ``e / d`` and ``q`` the other quotient; ``g = float32(p - y)``, ``h = float32(p * q)``.  A NaN ``x`` gives
    NaN ``g`` and ``h`` (which quantise to 0).

    ``"softmax"``: ``pred`` float64 ``[C, n]`` class-major, ``y`` int64 ``[n]`` class ids.  ``m = max_c x_c``, ``e_c =
    exp_neg(min(m - x_c, 708))``, ``S`` their sum in class order, ``p_c = e_c / S``; ``g_c = float32(p_c - [y == c])``,
    ``h_c = float32(p_c * (1 - p_c))``.  A row with a NaN or ``+inf`` margin is NaN throughout; a label outside ``[0,
    C)`` makes the row's ``2C`` outputs ``+0``: the row is ignored."""
    n, C = gbdt_args.grad(pred, y, loss)
    if loss == "squared":
        return (pred - y).to(torch.float32), torch.ones(n, dtype=torch.float32, device=pred.device)
    if loss == "logistic":
        e = _exp_neg(_clamp_t(pred.abs()))
        d = e + 1.0
        a, b = torch.ones_like(d) / d, e / d
        up = pred >= 0
        p, q = torch.where(up, a, b), torch.where(up, b, a)
        return (p - y).to(torch.float32), (p * q).to(torch.float32)
    m = pred[0]
    for c in range(1, C):
        x = pred[c]
        m = torch.where(m.isnan(), m, torch.where(x.isnan() | (x > m), x, m))
    e = [_exp_neg(_clamp_t(m - pred[c])) for c in range(C)]
    S = e[0]
    for c in range(1, C):
        S = S + e[c]
    live = (y >= 0) & (y < C)
    g, h = [], []
    for c in range(C):
        p = e[c] / S
        g.append(torch.where(live, p - (y == c).to(torch.float64), torch.zeros_like(p)))
        h.append(torch.where(live, p * (1.0 - p), torch.zeros_like(p)))
    return torch.stack(g).to(torch.float32), torch.stack(h).to(torch.float32)


def _give(result: torch.Tensor, out: Optional[torch.Tensor]) -> torch.Tensor:
    return result if out is None else out.copy_(result)


def gbdt_grad_absmax_torch(pred: torch.Tensor, y: torch.Tensor, loss: str, out: torch.Tensor = None) -> torch.Tensor:
    """``top`` float32 ``[C, 2]``: per class the ``g`` and the ``h`` of :func:`gbdt_grad_torch` with the largest key ``bits
    & 0x7fffffff`` - ``abs().max()`` with any NaN above infinity, 0 for ``n = 0``.  An integer maximum: the order of the
    rows cannot show.  On GPU tensors one call that stores no gradient."""
    n, C = gbdt_args.grad(pred, y, loss)
    if pred.is_cuda:
        from ..ops import device_ops
        return device_ops.gbdt_grad_absmax(pred, y, loss, out=out)
    keys = torch.stack([x.reshape(C, n).contiguous().view(torch.int32) & 0x7fffffff
                        for x in gbdt_grad_torch(pred, y, loss)], dim=1)                      # [C, 2, n]
    top = keys.max(dim=2).values if n else torch.zeros(C, 2, dtype=torch.int32)
    return _give(top.contiguous().view(torch.float32), out)


def gbdt_grad_quantize_torch(pred: torch.Tensor, y: torch.Tensor, loss: str, sg: torch.Tensor, sh: torch.Tensor,
                             out: torch.Tensor = None) -> torch.Tensor:
    """``gh`` int32 ``[C, n, 2]``: ``gh[c] = gbdt_quantize_torch(g[c], h[c], sg[c], sh[c])`` of :func:`gbdt_grad_torch`'s
    gradients, ``sg``, ``sh`` int32 ``[C]`` on the device of ``pred`` (a value outside ``+-MAX_SHIFT`` is clamped).  On GPU
    tensors one call in which the float gradients never reach memory and the shifts are read on the device."""
    n, C = gbdt_args.grad(pred, y, loss)
    gbdt_args.grad_shifts(sg, sh, C)
    if pred.is_cuda:
        from ..ops import device_ops
        return device_ops.gbdt_grad_quantize(pred, y, loss, sg, sh, out=out)
    g, h = (x.reshape(C, n) for x in gbdt_grad_torch(pred, y, loss))
    s = torch.stack([sg, sh]).clamp(-MAX_SHIFT, MAX_SHIFT).tolist()
    gh = torch.stack([gbdt_quantize_torch(g[c], h[c], s[0][c], s[1][c]) for c in range(C)])
    return _give(gh, out)


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


def grow_level(tree: Tree, nodes: List[int], rec, sg: int, sh: int, lam: float, lr: float, last: bool) -> List[int]:
    """Grow ``tree`` by one level on the host: ``nodes[i]`` is the tree node of histogram slot i and ``rec``
    the split record as lists (:class:`GbdtSplit`'s fields, slot i of each).  Every node takes its leaf
    value; it splits unless the level is the ``last``, ``H < 2`` or the record has no split (``f < 0``).
    The nodes are taken in ascending order whatever their slots, so the children are numbered the same
    for every grouping.  Returns the new frontier, empty when no node split."""
    frontier = []
    for i in sorted(range(len(nodes)), key=nodes.__getitem__):
        f, t = rec[1][i], rec[2][i]
        G, H = math.ldexp(rec[5][i], -sg), math.ldexp(rec[6][i], -sh)
        tree.value[nodes[i]] = -G / (H + lam) * lr
        if last or H < 2 or f < 0:
            continue
        left = tree.split(nodes[i], f, t)
        frontier += [left, left + 1]
    return frontier


def move_rows(bins: torch.Tensor, node_of: torch.Tensor, tree: Tree, nodes: List[int]) -> torch.Tensor:
    """The elementwise move of a level: a row of a node of ``nodes`` that split goes to the left child if
    ``bin <= threshold``, else to the right one (a missing-value bin goes right); every other row stays."""
    size = max(nodes) + 1                                   # the tree before this level grew
    feat_of, thr_of, left_of = [-1] * size, [0] * size, [0] * size
    for nd in nodes:
        if tree.left[nd] >= 0:
            feat_of[nd], thr_of[nd], left_of[nd] = tree.feature[nd], tree.threshold[nd], tree.left[nd]
    feat_of, thr_of, left_of = (torch.tensor(t, dtype=torch.int64).to(bins.device) for t in (feat_of, thr_of, left_of))
    f_row = feat_of[node_of]
    b_row = bins.gather(1, f_row.clamp(min=0)[:, None])[:, 0].to(torch.int64)
    child = left_of[node_of] + (b_row > thr_of[node_of]).to(torch.int64)
    return torch.where(f_row >= 0, child, node_of)


def next_segments(nodes: List[int], left: List[int], first_right: List[int]):
    """The partition level's table after a partition, on the host: ``nodes[i]`` is the tree node of segment
    i of k, ``left`` the grown tree's left children (-1: a final leaf, its rows were dropped),
    ``first_right[i]`` whether segment i's right child stands first.  Returns ``(parents, take,
    next_nodes)``: the segments that split, the entries of ``seg2`` that are the next table (the parents'
    first children, their second children, the end; the segments between are empty, so the table is
    contiguous and ``take[:kp + 1]`` is the table of the first children alone) and the tree node of every
    next segment."""
    k = len(nodes)
    parents = [i for i in range(k) if left[nodes[i]] >= 0]
    take = parents + [k + i for i in parents] + [2 * k]
    first = [left[nodes[i]] + first_right[i] for i in parents]
    second = [left[nodes[i]] + 1 - first_right[i] for i in parents]
    return parents, take, first + second


class _Levels:
    """How a tree's rows are grouped by node, level after level.  ``histograms`` gives the level's job-wide
    histograms and the tree node of every histogram slot; ``advance`` moves to the next level from the
    grown tree and the split record (lists)."""

    def __init__(self, comm, bins: torch.Tensor, gh: torch.Tensor, B: int):
        self.comm, self.bins, self.gh, self.B = comm, bins, gh, B
        self.nodes = [0]

    def _job_hist(self, rows, seg, out=None):
        hist = gbdt_hist_torch(self.bins, self.gh, rows, seg, self.B, out=out)
        _allreduce(self.comm, hist.view(-1), Operands.LONG_OPERAND(), Operators.Long.SUM)
        return hist


class _SortLevels(_Levels):
    """Every level sorts all rows by node (:func:`gbdt_level_rows`); the slots are the frontier in order."""

    def histograms(self, tree: Tree, node_of: torch.Tensor):
        k = len(self.nodes)
        slot_of_node = torch.full((len(tree.value),), -1, dtype=torch.int64)
        slot_of_node[self.nodes] = torch.arange(k)
        return self._job_hist(*gbdt_level_rows(node_of, slot_of_node.to(node_of.device), k)), self.nodes

    def advance(self, tree: Tree, rec) -> None:
        self.nodes = [c for nd in self.nodes if tree.left[nd] >= 0 for c in (tree.left[nd], tree.right[nd])]


class _PartitionLevels(_Levels):
    """The rows stay grouped from level to level: every segment is split in two by
    :func:`gbdt_partition_torch` (K17) into the other of two row buffers, and :func:`next_segments` says
    which entries of ``seg2`` are the next table.  With ``subtract`` the child with the smaller hessian mass
    stands first, only the first children are histogrammed and allreduced, and every sibling is parent -
    child."""

    def __init__(self, comm, bins, gh, B, subtract: bool):
        super().__init__(comm, bins, gh, B)
        n, dev = bins.shape[0], bins.device
        self.subtract = subtract
        self.rows = torch.arange(n, dtype=torch.int32, device=dev)
        self.spare = torch.empty(n, dtype=torch.int32, device=dev)      # the two row buffers take turns
        self.seg = torch.tensor([0, n], dtype=torch.int64, device=dev)
        self.parents, self.hist = [], None                  # of the level before: what the siblings are taken from

    def histograms(self, tree: Tree, node_of: torch.Tensor):
        kp = len(self.parents)
        if self.subtract and kp:
            both = torch.empty((2 * kp,) + tuple(self.hist.shape[1:]), dtype=torch.int64, device=self.bins.device)
            self._job_hist(self.rows, self.seg[:kp + 1], out=both[:kp])
            parent_of = torch.tensor(self.parents, dtype=torch.int32, device=self.bins.device)
            gbdt_hist_subtract_torch(self.hist, both[:kp], parent_of, out=both[kp:])
            self.hist = both
        else:
            self.hist = self._job_hist(self.rows, self.seg)
        return self.hist, self.nodes

    def advance(self, tree: Tree, rec) -> None:
        k, dev = len(self.nodes), self.bins.device
        feature = [tree.feature[nd] for nd in self.nodes]   # -1: a final leaf
        # right first iff it has the smaller hessian mass, by the allreduced record: the same on every rank
        first_right = [int(self.subtract and f >= 0 and rec[6][i] - rec[4][i] < rec[4][i])
                       for i, f in enumerate(feature)]
        up = torch.tensor([feature, [tree.threshold[nd] for nd in self.nodes], first_right], dtype=torch.int32).to(dev)
        seg2 = torch.empty(2 * k + 1, dtype=torch.int64, device=dev)
        gbdt_partition_torch(self.bins, self.rows, self.seg, up[0], up[1], up[2], out=(self.spare, seg2))
        self.rows, self.spare = self.spare, self.rows
        self.parents, take, self.nodes = next_segments(self.nodes, tree.left, first_right)
        self.seg = seg2[torch.tensor(take).to(dev)]


def _check_modes(level: str, subtract: bool, update: str) -> None:
    if level not in ("sort", "partition"):
        raise ValueError(f"level {level!r} must be 'sort' or 'partition'")
    if subtract and level != "partition":
        raise ValueError("subtract=True needs level='partition'")
    if update not in ("rows", "walk"):
        raise ValueError(f"update {update!r} must be 'rows' or 'walk'")
    if update == "walk" and level != "partition":
        raise ValueError("update='walk' needs level='partition'")


def _grow_tree(comm, bins, gh, pred, B, sg, sh, depth, lr, lam, level, subtract, update):
    """``(tree, pred)``: one tree grown level by level on the quantised ``gh`` int32 ``[n, 2]``, and ``pred`` float64
    ``[n]`` with the tree's values added as ``update`` says (in place for ``"rows"``, a new tensor for ``"walk"``)."""
    n, dev = bins.shape[0], bins.device
    levels = _PartitionLevels(comm, bins, gh, B, subtract) if level == "partition" else \
        _SortLevels(comm, bins, gh, B)
    node_of = torch.zeros(n, dtype=torch.int64, device=dev) if update == "rows" else None
    tree = Tree([-1], [-1], [-1], [-1], [0.0])
    for level_no in range(depth + 1):
        hist, nodes = levels.histograms(tree, node_of)
        rec = [t.tolist() for t in gbdt_split_torch(hist, sg, sh, lam)]
        if not grow_level(tree, nodes, rec, sg, sh, lam, lr, last=level_no == depth):
            break
        levels.advance(tree, rec)
        if update == "rows":
            node_of = move_rows(bins, node_of, tree, nodes)
    if update == "rows":
        pred += torch.tensor(tree.value, dtype=torch.float64, device=dev)[node_of]
    else:
        pred = gbdt_predict_torch(bins, pack_forest([tree], dev), init=pred)
    return tree, pred


def train_gbdt_quantized(comm, bins: torch.Tensor, y: torch.Tensor, B: int, trees: int = 5, depth: int = 3,
                         lr: float = 0.3, lam: float = 1.0, level: str = "sort", subtract: bool = False,
                         update: str = "rows", loss: str = "squared", classes: Optional[int] = None) -> List[Tree]:
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
    grow the default's trees bit for bit.

    ``update`` is how a finished tree reaches ``pred``: ``"rows"`` moves ``node_of`` elementwise after every level
    (:func:`move_rows`) and adds ``value[node_of]``; ``"walk"`` (``level="partition"`` only, which never reads
    ``node_of``) keeps no ``node_of`` and walks the finished tree once with :func:`gbdt_predict_torch` (K18).  The
    walk ends on the leaf ``node_of`` would hold and adds the same float64, so the trees are the same bit for
    bit.

    ``loss`` is ``"squared"`` (the above), ``"logistic"`` (``y`` in ``[0, 1]``, the trees sum to a log-odds margin) or
    ``"softmax"`` (``y`` int64 class ids and ``classes=C``, which goes with softmax alone; ``C`` trees a round, returned
    round-major: tree ``t * C + c`` adds to class c's margin, see :func:`predict_gbdt`).  The last two are
    :func:`train_gbdt_fused`."""
    if loss != "squared" or classes is not None:
        return train_gbdt_fused(comm, bins, y, B, loss, classes, trees, depth, lr, lam, level, subtract, update)
    _check_modes(level, subtract, update)
    dev = bins.device
    n = bins.shape[0]
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
        tree, pred = _grow_tree(comm, bins, gh, pred, B, sg, sh, depth, lr, lam, level, subtract, update)
        out.append(tree)
    return out


def train_gbdt_fused(comm, bins: torch.Tensor, y: torch.Tensor, B: int, loss: str, classes: Optional[int] = None,
                     trees: int = 5, depth: int = 3, lr: float = 0.3, lam: float = 1.0, level: str = "sort",
                     subtract: bool = False, update: str = "rows") -> List[Tree]:
    """:func:`train_gbdt_quantized` for any loss of :func:`gbdt_grad_torch`, over the fused gradient ops (K21): the
    margins ``pred`` float64 ``[C, n]`` stay class-major on the device of ``bins`` and per round there is one
    :func:`gbdt_grad_absmax_torch`, one allreduce MAX of its ``2C`` values as doubles (a NaN counts as infinity),
    :func:`gbdt_shift` per class, one :func:`gbdt_grad_quantize_torch` with the shifts as a device tensor, and then
    for ``c = 0 .. C - 1`` one tree grown on ``gh[c]`` by the level machinery of :func:`train_gbdt_quantized`, which
    updates ``pred[c]``.  ``trees`` is the number of rounds; tree ``t * C + c`` of the result is round t's tree of class
    c.  ``"logistic"`` and ``"squared"`` have ``C = 1``; ``"squared"`` grows the trees of :func:`train_gbdt_quantized`'s
    default bit for bit.  Every gradient is per row and specified to the bit, every sum is in integers: the trees do
    not depend on the rank count or the device."""
    _check_modes(level, subtract, update)
    if (loss == "softmax") != (classes is not None):
        raise ValueError("classes is required with loss='softmax' and goes with no other loss")
    dev, n = bins.device, bins.shape[0]
    C = classes if loss == "softmax" else 1
    if isinstance(C, bool) or not isinstance(C, int) or not 1 <= C <= gbdt_args.MAX_CLASSES:
        raise ValueError(f"classes {C!r} must be an int in [1, {gbdt_args.MAX_CLASSES}]")
    y = y.to(device=dev, dtype=torch.int64 if loss == "softmax" else torch.float64)
    pred = torch.zeros((C, n) if loss == "softmax" else (n,), dtype=torch.float64, device=dev)
    gbdt_args.grad(pred, y, loss, classes)
    margins = pred.view(C, n)
    top = torch.empty(C, 2, dtype=torch.float32, device=dev)
    gh = torch.empty(C, n, 2, dtype=torch.int32, device=dev)
    out: List[Tree] = []
    for _ in range(trees):
        gbdt_grad_absmax_torch(pred, y, loss, out=top)
        job = torch.nan_to_num(top.double().view(-1), nan=math.inf)
        job = _allreduce(comm, job, Operands.DOUBLE_OPERAND(), Operators.Double.MAX).tolist()
        shifts = [[gbdt_shift(job[2 * c + j]) for c in range(C)] for j in (0, 1)]
        on_dev = torch.tensor(shifts, dtype=torch.int32).to(dev)
        gbdt_grad_quantize_torch(pred, y, loss, on_dev[0], on_dev[1], out=gh)
        for c in range(C):
            tree, moved = _grow_tree(comm, bins, gh[c], margins[c], B, shifts[0][c], shifts[1][c], depth, lr, lam, level,
                                     subtract, update)
            if moved.data_ptr() != margins[c].data_ptr():          # update="walk" gives a new tensor
                margins[c].copy_(moved)
            out.append(tree)
    return out
