"""The argument rules of the fixed-point GBDT ops (K16 - K21) and the limits behind them, stated once:
the definitions of :mod:`mp4x.parallel.gbdt` and the wrappers of :mod:`mp4x.ops.device_ops` both call
the op's function here, which checks what both forms require and returns the sizes.  What only the
device requires (GPU tensors, sizes below ``2**31``, alignment, the node caps, ``out=``) stays with the
wrapper.  Torch only: importing this loads no native library.  tests/test_native_abi_cpu.py compares the
limits with csrc/kernels/gbdt_hist_map.hpp and gbdt_part_map.hpp."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

MAX_SHIFT = 200                      # kMaxShift: float64(x) * 2**s is exact for every float32 x
MAX_NODES = 4096                     # kMaxNodes: a histogram table fits one block's LDS
MAX_PARENTS = MAX_NODES // 2         # kMaxParents: the 2k children stay a histogram table
MAX_BINS = 256                       # kMaxBins: bins are bytes
QMAX = 2 ** 31 - 1                   # a quantised gradient or hessian is clamped to +-QMAX
MAX_STEPS = 64                       # kMaxSteps (gbdt_walk_map.hpp): the longest root-to-leaf path, in edges
MAX_EDGES = 255                      # kMaxEdges (gbdt_bin_map.hpp): a position among the edges is a byte
MAX_CLASSES = 64                     # kMaxClasses (gbdt_loss_map.hpp): a block's key table is 2 * 64 words
LOSSES = ("squared", "logistic", "softmax")      # a loss's code in the native calls is its index


def shifts(*s) -> None:
    for x in s:
        if isinstance(x, bool) or not isinstance(x, int) or abs(x) > MAX_SHIFT:
            raise ValueError(f"the shift {x!r} is not an int in [-{MAX_SHIFT}, {MAX_SHIFT}]")


def _table(rows: torch.Tensor, seg: torch.Tensor) -> Tuple[int, int]:
    if rows.dtype != torch.int32 or rows.dim() != 1 or seg.dtype != torch.int64 or seg.dim() != 1 or seg.numel() < 1:
        raise ValueError("rows must be int32 [m] and seg int64 [k + 1]")
    return rows.numel(), seg.numel() - 1


def quantize(g: torch.Tensor, h: torch.Tensor, sg: int, sh: int) -> int:
    """``n``."""
    shifts(sg, sh)
    if g.dtype != torch.float32 or h.dtype != torch.float32 or g.dim() != 1 or h.shape != g.shape:
        raise ValueError("g and h must be float32 [n]")
    return g.numel()


def histogram(bins: torch.Tensor, gh: torch.Tensor, rows: torch.Tensor, seg: torch.Tensor, B: int):
    """``(n, F, m, k)``.  ``F = 0`` is the definition's to accept (an empty histogram) and the wrapper's to
    refuse."""
    if isinstance(B, bool) or not isinstance(B, int) or not 2 <= B <= MAX_BINS:
        raise ValueError(f"B {B!r} must be an int in [2, {MAX_BINS}]")
    if bins.dtype != torch.uint8 or bins.dim() != 2 or gh.dtype != torch.int32 or tuple(gh.shape) != (bins.shape[0], 2):
        raise ValueError("bins must be uint8 [n, F] and gh int32 [n, 2]")
    return tuple(bins.shape) + _table(rows, seg)


def split(hist: torch.Tensor, sg: int, sh: int):
    """``(k, F, B)``.  ``B <= MAX_BINS`` is the kernel's limit and stays with the wrapper."""
    shifts(sg, sh)
    if hist.dtype != torch.int64 or hist.dim() != 4 or hist.shape[3] != 2 or hist.shape[1] < 1 or hist.shape[2] < 2:
        raise ValueError("hist must be int64 [k, F, B, 2] with F >= 1 and B >= 2")
    return tuple(hist.shape[:3])


def partition(bins: torch.Tensor, rows: torch.Tensor, seg: torch.Tensor, feature: torch.Tensor,
              threshold: torch.Tensor, first_right: Optional[torch.Tensor]):
    """``(n, F, m, k)``; ``first_right`` may be None (no node puts its right child first)."""
    if bins.dtype != torch.uint8 or bins.dim() != 2 or bins.shape[1] < 1:
        raise ValueError("bins must be uint8 [n, F] with F >= 1")
    m, k = _table(rows, seg)
    records = (feature, threshold) + (() if first_right is None else (first_right,))
    if k > MAX_PARENTS or any(t.dtype != torch.int32 or tuple(t.shape) != (k,) for t in records):
        raise ValueError(f"feature, threshold and first_right must be int32 [k] with k <= {MAX_PARENTS}")
    return tuple(bins.shape) + (m, k)


def subtract(parent: torch.Tensor, small: torch.Tensor, parent_of: torch.Tensor):
    """``(k, kp, cells)`` with ``cells = F * B``."""
    if parent.dtype != torch.int64 or parent.dim() != 4 or parent.shape[3] != 2 or small.dtype != torch.int64 or \
            small.dim() != 4 or small.shape[1:] != parent.shape[1:] or parent_of.dtype != torch.int32 or \
            tuple(parent_of.shape) != (small.shape[0],):
        raise ValueError("parent must be int64 [k, F, B, 2], small int64 [kp, F, B, 2] and parent_of int32 [kp]")
    return parent.shape[0], small.shape[0], parent.shape[1] * parent.shape[2]


def _walk(rows: torch.Tensor, nodes: torch.Tensor, value: torch.Tensor, tree_off: torch.Tensor, steps: int,
          init: Optional[torch.Tensor]):
    """``(n, F, T, N)`` of a forest walk over ``rows`` ``[n, F]``, whose own rule the caller has checked."""
    if nodes.dtype != torch.int32 or nodes.dim() != 2 or nodes.shape[1] != 4 or value.dtype != torch.float64 or \
            tuple(value.shape) != (nodes.shape[0],) or tree_off.dtype != torch.int32 or tree_off.dim() != 1 or \
            tree_off.numel() < 1:
        raise ValueError("nodes must be int32 [N, 4], value float64 [N] and tree_off int32 [T + 1]")
    if isinstance(steps, bool) or not isinstance(steps, int) or not 0 <= steps <= MAX_STEPS:
        raise ValueError(f"steps {steps!r} must be an int in [0, {MAX_STEPS}]")
    if init is not None and (init.dtype != torch.float64 or tuple(init.shape) != (rows.shape[0],)):
        raise ValueError("init must be float64 [n]")
    return tuple(rows.shape) + (tree_off.numel() - 1, nodes.shape[0])


def predict(bins: torch.Tensor, nodes: torch.Tensor, value: torch.Tensor, tree_off: torch.Tensor, steps: int,
            init: Optional[torch.Tensor]):
    """``(n, F, T, N)``; ``init`` may be None (the sums start at ``+0.0``)."""
    if bins.dtype != torch.uint8 or bins.dim() != 2 or bins.shape[1] < 1:
        raise ValueError("bins must be uint8 [n, F] with F >= 1")
    return _walk(bins, nodes, value, tree_off, steps, init)


def features(X: torch.Tensor):
    """``(n, F)``."""
    if X.dtype not in (torch.float32, torch.float16, torch.bfloat16) or X.dim() != 2:
        raise ValueError("X must be float32, float16 or bfloat16 [n, F]")
    return tuple(X.shape)


def predict_float(X: torch.Tensor, nodes: torch.Tensor, value: torch.Tensor, tree_off: torch.Tensor, steps: int,
                  init: Optional[torch.Tensor]):
    """``(n, F, T, N)`` of the walk over float features (K20): :func:`predict`'s rules with ``X`` for ``bins``."""
    if features(X)[1] < 1:
        raise ValueError("X must have F >= 1 features")
    return _walk(X, nodes, value, tree_off, steps, init)


def float_forest(nodes: torch.Tensor, edges: torch.Tensor, cnt: torch.Tensor):
    """``(F, E)`` of the edges a forest's bin thresholds are turned into keys with."""
    if nodes.dtype != torch.int32 or nodes.dim() != 2 or nodes.shape[1] != 4:
        raise ValueError("nodes must be int32 [N, 4]")
    if edges.dtype != torch.float32 or edges.dim() != 2 or edges.shape[0] < 1 or edges.shape[1] > MAX_EDGES:
        raise ValueError(f"edges must be float32 [F, E] with F >= 1 and E <= {MAX_EDGES}")
    if cnt.dtype != torch.int32 or tuple(cnt.shape) != (edges.shape[0],):
        raise ValueError("cnt must be int32 [F]")
    return tuple(edges.shape)


def edges(X: torch.Tensor, B: int):
    """``(n, F)``; ``B - 1 <= MAX_EDGES``."""
    if isinstance(B, bool) or not isinstance(B, int) or not 2 <= B <= MAX_EDGES + 1:
        raise ValueError(f"B {B!r} must be an int in [2, {MAX_EDGES + 1}]")
    return features(X)


def bin(X: torch.Tensor, edges: torch.Tensor, cnt: torch.Tensor, missing: int):
    """``(n, F, E)``."""
    F = features(X)[1]
    if edges.dtype != torch.float32 or edges.dim() != 2 or edges.shape[0] != F or edges.shape[1] > MAX_EDGES:
        raise ValueError(f"edges must be float32 [F, E] with E <= {MAX_EDGES}")
    if cnt.dtype != torch.int32 or tuple(cnt.shape) != (F,):
        raise ValueError("cnt must be int32 [F]")
    if isinstance(missing, bool) or not isinstance(missing, int) or not 0 <= missing <= 255:
        raise ValueError(f"missing {missing!r} must be an int in [0, 255]")
    return X.shape[0], F, edges.shape[1]


def grad(pred: torch.Tensor, y: torch.Tensor, loss: str, classes: Optional[int] = None):
    """``(n, C)`` of the margins of a loss (K21): ``pred`` float64 ``[n]`` and ``y`` float64 ``[n]``, or for
    ``"softmax"`` ``pred`` float64 ``[C, n]`` class-major, ``1 <= C <= MAX_CLASSES``, and ``y`` int64 ``[n]``.  ``classes``
    may be given with ``"softmax"`` alone and is then ``C``."""
    if loss not in LOSSES:
        raise ValueError(f"loss {loss!r} must be one of {LOSSES}")
    soft = loss == "softmax"
    if classes is not None and (not soft or isinstance(classes, bool) or not isinstance(classes, int)):
        raise ValueError(f"classes {classes!r} goes with loss='softmax' alone and is an int")
    if pred.dtype != torch.float64 or pred.dim() != (2 if soft else 1):
        raise ValueError("pred must be float64 [n], for softmax float64 [C, n]")
    n, C = pred.shape[-1], pred.shape[0] if soft else 1
    if not 1 <= C <= MAX_CLASSES or classes not in (None, C):
        raise ValueError(f"pred holds {C} classes: at least 1, at most {MAX_CLASSES}, and classes={classes!r} if given")
    if y.dtype != (torch.int64 if soft else torch.float64) or tuple(y.shape) != (n,):
        raise ValueError("y must be float64 [n], for softmax int64 [n]")
    return n, C


def grad_shifts(sg: torch.Tensor, sh: torch.Tensor, C: int) -> None:
    if any(s.dtype != torch.int32 or tuple(s.shape) != (C,) for s in (sg, sh)):
        raise ValueError("sg and sh must be int32 [C]")
