"""Expert-parallel token dispatch / combine on the ragged all-to-all.

``dispatch`` turns ``T x K`` (token, expert) assignments into rows grouped by local expert on the
rank that owns the expert; ``combine`` brings every expert's output rows back and sums each
token's K rows with its gate weights.  Rank ``r`` of ``p`` owns experts ``[r*E/p, (r+1)*E/p)``.

Layout contract (``tests/moe_ref.py`` holds it in plain torch):

* send order = the stable sort of the flattened assignments ``a = t*K + k`` by expert id
  (``slots[a]`` = position, -1 for a dropped assignment).  Experts are owned in contiguous ascending
  blocks, so this order is already grouped by destination rank.
* the all-to-all returns rows grouped by source rank, inside a source by expert, inside that in
  the sender's order; one segment copy regroups them expert-major (expert, then source rank, then
  sender order).  With one local expert the two orders coincide and the copy is skipped.
* the way back is the inverse copy and the all-to-all with the transposed count matrix, which
  lands rows in the sender's slot order; the combine then reads them through ``slots``, k by k,
  ``acc = acc + w * x`` in f32 with two roundings per step and one rounding to the dtype at the
  end: no atomics, identical run to run and to the CPU reference.

One exchange of ``E + 2`` counts per rank (per-expert rows, dropped ids, ids >= E) through
``sparse._count_matrix`` serves the dispatch, every later combine and both backward passes.

Expert capacity (``capacity`` / ``capacity_factor``): expert e accepts the first C assignments in
the global order (source rank, then the sender's flattened assignment index).  After the count
exchange every rank holds the whole demand matrix ``D[i][e]``, so the rows of expert e that rank i
may keep, ``keep[i][e] = min(D[i][e], max(0, C - sum_{j<i} D[j][e]))`` (:func:`capacity_quota`),
cost no further exchange; the scatter half of the route compares an assignment's position inside
its expert with that quota and gives a clipped assignment slot -1.  A capped call is, bit for bit,
the uncapped call on the ids with every clipped assignment replaced by -1: clipped rows are never
read, written or sent, every later combine skips them, and both backward passes follow the plan.

GPU tensors run the K9 kernels (``csrc/kernels/moe.hip``); host tensors, and GPU tensors where
the native library is absent, run the torch implementation of the same contract below.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import torch

from ..exceptions import Mp4jException

MAX_EXPERTS = 2048
DTYPES = (torch.float32, torch.bfloat16, torch.float16)


class TokenPlan:
    """What one ``dispatchTokens`` call learned; read-only, reusable for any number of combines
    and for the backward passes.

    ``num_tokens`` / ``top_k`` / ``num_experts``: the call's T, K and E.  ``expert_counts``: rows
    of every local expert (the groups of the dispatched rows, ascending).  ``send_counts`` /
    ``recv_counts``: rows to / from every rank.  ``slots``: int64 ``[T*K]`` on the tokens' device.
    ``matrix[i][j]``: rows rank i sends to rank j.  ``expert_matrix[i][e]``: rows rank i sends to
    global expert e.

    With an expert capacity all of the above describe the rows that stayed.  ``capacity``: the
    resolved C of the call (None: no capacity).  ``demand_matrix[i][e]``: the assignments of rank i
    with expert e before clipping (``expert_matrix`` itself when there is no capacity): what a
    load-balancing loss or a monitor wants.  ``clipped``: this rank's assignments the capacity
    dropped, ``sum_e demand_matrix[r][e] - expert_matrix[r][e]``."""
    __slots__ = ("num_tokens", "top_k", "num_experts", "expert_counts", "send_counts", "recv_counts", "slots",
                 "matrix", "expert_matrix", "row_shape", "dtype", "rank", "capacity", "demand_matrix", "clipped",
                 "_route", "_clip", "_frozen")

    def __init__(self, **kw):
        kw = {"capacity": None, "demand_matrix": kw.get("expert_matrix"), "clipped": 0, "_clip": None, **kw}
        for k, v in kw.items():
            object.__setattr__(self, k, v)
        object.__setattr__(self, "_frozen", True)

    def __setattr__(self, name, value):
        raise AttributeError("TokenPlan is read-only")

    @property
    def num_rows(self) -> int:
        return sum(self.expert_counts)


def _native_ok(t: torch.Tensor) -> bool:
    if not t.is_cuda:
        return False
    from ..ops import native
    return native.available()


def _width(shape: Sequence[int]) -> int:
    w = 1
    for d in shape:
        w *= int(d)
    return w


def _check_rows(what: str, t: torch.Tensor):
    if not isinstance(t, torch.Tensor):
        raise Mp4jException(f"{what} needs a torch tensor")
    if t.dim() < 1 or not t.is_contiguous():
        raise Mp4jException(f"{what}: rows must be a contiguous [rows, ...] tensor")
    if t.dtype not in DTYPES:
        raise Mp4jException(f"{what}: dtype {t.dtype} is not float32 / bfloat16 / float16")
    rb = _width(t.shape[1:]) * t.element_size()
    if rb == 0 or (t.is_cuda and rb % 16):
        raise Mp4jException(f"{what}: rows of {rb} bytes on a GPU tensor are not whole 16-byte vectors")
    if t.is_cuda:
        from ..ops.native import capturing_now
        if capturing_now():
            raise Mp4jException(f"{what} inside a graph capture: the count exchange is a host sync")


# ---------------------------------------------------------------- the torch form of the kernels
def _torch_route(ids: torch.Tensor, nb: int):
    """(counts int64[nb + 2], slots int64[n], order of the placed assignments)."""
    ids = ids.to(torch.int64)
    n = ids.numel()
    neg, over = ids < 0, ids >= nb
    placed = ~(neg | over)
    counts = torch.cat([torch.bincount(ids[placed], minlength=nb),
                        torch.stack([neg.sum(), over.sum()]).to(torch.int64)])
    order = torch.argsort(torch.where(placed, ids, torch.full_like(ids, nb)), stable=True)[:int(placed.sum())]
    slots = torch.full((n,), -1, dtype=torch.int64, device=ids.device)
    slots[order] = torch.arange(order.numel(), dtype=torch.int64, device=ids.device)
    return counts, slots, order


def _torch_scatter(x: torch.Tensor, order: torch.Tensor, top_k: int, row_scale: Optional[torch.Tensor]):
    rows = x[order // top_k]
    if row_scale is None:
        return rows
    s = row_scale.reshape(-1)[order].view((-1,) + (1,) * (x.dim() - 1))
    return (s * rows.to(torch.float32)).to(x.dtype)


def _torch_combine(rows: torch.Tensor, slots: torch.Tensor, weights: Optional[torch.Tensor], T: int, K: int):
    shape = (T,) + tuple(rows.shape[1:])
    acc = torch.zeros(shape, dtype=torch.float32, device=rows.device)
    if rows.shape[0] and T:
        sl = slots.view(T, K)
        bshape = (T,) + (1,) * (rows.dim() - 1)
        for k in range(K):
            s = sl[:, k]
            xk = rows[s.clamp(min=0)].to(torch.float32)
            if weights is not None:
                xk = weights.view(T, K)[:, k].view(bshape) * xk          # one rounding ...
            acc = torch.where((s >= 0).view(bshape), acc + xk, acc)      # ... then another: never an FMA
    return acc.to(rows.dtype)


def _torch_clip(route, ids: torch.Tensor, nb: int, keep: Sequence[int]):
    """``_torch_route``'s result under the quota ``keep[e]``: the assignments past it leave the
    slots and the order; the others close ranks (still the stable sort)."""
    counts, slots, order = route
    keep_t = torch.tensor(list(keep), dtype=torch.int64, device=ids.device)
    start = torch.cumsum(counts[:nb], 0) - counts[:nb]
    e = ids.to(torch.int64)[order]
    pe = torch.arange(order.numel(), dtype=torch.int64, device=ids.device) - start[e]
    order = order[pe < keep_t[e]]
    slots = torch.full_like(slots, -1)
    slots[order] = torch.arange(order.numel(), dtype=torch.int64, device=ids.device)
    return counts, slots, order


# ---------------------------------------------------------------- expert capacity
def capacity_quota(demand: Sequence[Sequence[int]], capacity: int) -> Tuple[Tuple[int, ...], ...]:
    """``keep[i][e] = min(D[i][e], max(0, C - sum_{j<i} D[j][e]))``: the rows of expert e that rank
    i keeps when every expert accepts the first ``capacity`` assignments in (rank, assignment)
    order.  A pure function of the demand matrix ``D[i][e]``, the same on every rank."""
    C = int(capacity)
    keep, used = [], [0] * (len(demand[0]) if len(demand) else 0)
    for row in demand:
        keep.append(tuple(min(int(d), max(0, C - u)) for d, u in zip(row, used)))
        used = [u + int(d) for d, u in zip(row, used)]
    return tuple(keep)


def _check_capacity(capacity, capacity_factor):
    """The caller's contract, the same on every rank: refused before the count exchange."""
    if capacity is not None and capacity_factor is not None:
        raise Mp4jException("dispatchTokens: give capacity or capacityFactor, not both")
    if capacity is not None and (isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < 1):
        raise Mp4jException(f"dispatchTokens: capacity {capacity!r} is not an int >= 1")
    if capacity_factor is not None:
        f = capacity_factor
        if isinstance(f, bool) or not isinstance(f, (int, float)) or not math.isfinite(f) or f <= 0:
            raise Mp4jException(f"dispatchTokens: capacityFactor {f!r} is not a finite float > 0")


def _resolve_capacity(capacity, capacity_factor, assignments: int, E: int) -> Optional[int]:
    """C of the call: ``capacity`` itself, or ``max(1, ceil(f * N / E))`` with N the assignments
    of all ranks (negative ids included), which the count exchange gave every rank."""
    if capacity_factor is not None:
        return max(1, math.ceil(float(capacity_factor) * assignments / E))
    return capacity


# ---------------------------------------------------------------- count matrix, regroup
def _segments(plan: TokenPlan) -> List[Tuple[int, int, int]]:
    """(expert-major row offset, source-major row offset, rows) of every (source, local expert)
    segment this rank receives."""
    p = len(plan.matrix)
    el = plan.num_experts // p
    lo = plan.rank * el
    seg = [[plan.expert_matrix[i][lo + e] for e in range(el)] for i in range(p)]
    out, src = [], 0
    ebase = [0] * el
    for e in range(1, el):
        ebase[e] = ebase[e - 1] + plan.expert_counts[e - 1]
    fill = list(ebase)
    for i in range(p):
        for e in range(el):
            c = seg[i][e]
            if c:
                out.append((fill[e], src, c))
            fill[e] += c
            src += c
    return out


def _regroup(rows: torch.Tensor, plan: TokenPlan, inverse: bool) -> torch.Tensor:
    """Source-major -> expert-major (or back): one segment copy; nothing to do with one local expert."""
    if plan.num_experts // len(plan.matrix) == 1 or len(plan.matrix) == 1 or rows.shape[0] == 0:
        return rows
    w = _width(rows.shape[1:])
    segs = _segments(plan)
    out = torch.empty_like(rows)
    if _native_ok(rows):
        from ..ops.device_ops import segment_copy_
        segment_copy_(out, rows, [((s if inverse else d) * w, (d if inverse else s) * w, c * w) for d, s, c in segs])
        return out
    for d, s, c in segs:
        if inverse:
            out[s:s + c] = rows[d:d + c]
        else:
            out[d:d + c] = rows[s:s + c]
    return out


def _exchange(engine, send: torch.Tensor, send_counts, mat, operand):
    """The all-to-all with a count matrix every rank already holds (no count exchange)."""
    if send.is_cuda:
        got, _ = engine.all_to_all_v(send, list(send_counts), None, operand, mat=mat)
        return got
    # host tensors: the backend moves bytes (gloo has no 16-bit float all-to-all everywhere)
    n, shape = send.shape[0], tuple(send.shape[1:])
    raw = send.reshape(n, _width(shape)).view(torch.uint8)
    got, _ = engine.all_to_all_v(raw, list(send_counts), None, operand, mat=mat)
    return got.view(send.dtype).view((got.shape[0],) + shape)


# ---------------------------------------------------------------- dispatch
def _route_rows(x: torch.Tensor, plan_route, top_k: int, placed: int, row_scale: Optional[torch.Tensor],
                clip: Optional[torch.Tensor] = None):
    """Rows of ``x`` replicated into send order (the second half of the route).  ``clip``: the
    device ``[keep | kept_base]`` of a capped call (the torch form's route is clipped already)."""
    if _native_ok(x):
        from ..ops.device_ops import moe_route_scatter
        out = torch.empty((placed,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
        slots = moe_route_scatter(plan_route, x, top_k, out, row_scale=row_scale, placed=placed, clip=clip)
        return out, slots
    _, slots, order = plan_route
    return _torch_scatter(x, order, top_k, row_scale), slots


def dispatch(engine, x: torch.Tensor, expert_ids: torch.Tensor, num_experts: int, operand=None, capacity=None,
             capacity_factor=None):
    """``(rows, plan)``: see ``ProcessCommSlave.dispatchTokens``."""
    p, r = engine.p, engine.rank
    E = int(num_experts)
    _check_rows("dispatchTokens", x)
    _check_capacity(capacity, capacity_factor)
    if E < 1 or E % p:
        raise Mp4jException(f"dispatchTokens: numExperts {E} is not a positive multiple of the {p} ranks")
    if E > MAX_EXPERTS:
        raise Mp4jException(f"dispatchTokens: numExperts {E} > {MAX_EXPERTS}")
    if not isinstance(expert_ids, torch.Tensor) or expert_ids.dtype not in (torch.int32, torch.int64):
        raise Mp4jException("dispatchTokens: expertIds must be an int32 / int64 tensor")
    T = x.shape[0]
    if expert_ids.dim() not in (1, 2) or expert_ids.shape[0] != T or expert_ids.device != x.device:
        raise Mp4jException(f"dispatchTokens: expertIds {tuple(expert_ids.shape)} on {expert_ids.device} does not "
                            f"match {T} tokens on {x.device}")
    K = 1 if expert_ids.dim() == 1 else int(expert_ids.shape[1])
    if K < 1:
        raise Mp4jException("dispatchTokens: expertIds needs at least one column")
    ids = expert_ids.reshape(-1).contiguous()
    native = _native_ok(x)
    # 1. route count
    if native:
        from ..ops.device_ops import moe_route_count
        route = moe_route_count(ids, E)
        counts = route.counts
    else:
        route = _torch_route(ids, E)
        counts = route[0]
    # 2. the one count exchange: E + 2 numbers per rank
    if p > 1:
        from . import sparse
        rows_ = sparse._count_matrix(engine, counts)
    else:
        rows_ = [counts.tolist()]
    emat = tuple(tuple(int(v) for v in row[:E]) for row in rows_)
    bad = [(j, int(row[E + 1])) for j, row in enumerate(rows_) if row[E + 1]]
    if bad:
        raise Mp4jException(f"dispatchTokens: rank {bad[0][0]} has {bad[0][1]} expert id(s) >= numExperts {E}")
    # an expert capacity: every rank works out every rank's quota from the demand matrix
    demand, clip, clipped = emat, None, 0
    C = _resolve_capacity(capacity, capacity_factor, sum(int(v) for row in rows_ for v in row[:E + 1]), E)
    if C is not None:
        emat = capacity_quota(demand, C)
        keep = emat[r]
        clipped = sum(demand[r]) - sum(keep)
        if native:
            kbase = [0] * E
            for e in range(1, E):
                kbase[e] = kbase[e - 1] + keep[e - 1]
            clip = torch.tensor(list(keep) + kbase, dtype=torch.int64).to(x.device)      # one small H2D copy
        else:
            route = _torch_clip(route, ids, E, keep)
    el = E // p
    mat = tuple(tuple(sum(emat[i][j * el:(j + 1) * el]) for j in range(p)) for i in range(p))
    send_counts = mat[r]
    recv_counts = tuple(mat[i][r] for i in range(p))
    expert_counts = tuple(sum(emat[i][r * el + e] for i in range(p)) for e in range(el))
    # 3. route scatter
    send, slots = _route_rows(x, route, K, sum(send_counts), None, clip)
    plan = TokenPlan(num_tokens=T, top_k=K, num_experts=E, expert_counts=expert_counts, send_counts=send_counts,
                     recv_counts=recv_counts, slots=slots, matrix=mat, expert_matrix=emat,
                     row_shape=tuple(x.shape[1:]), dtype=x.dtype, rank=r, capacity=C, demand_matrix=demand,
                     clipped=clipped, _route=route, _clip=clip)
    # 4. the all-to-all with that matrix, 5. expert-major
    return _forward_rows(engine, send, plan, operand), plan


def _forward_rows(engine, send: torch.Tensor, plan: TokenPlan, operand):
    if len(plan.matrix) == 1:
        return send                         # one rank: send order is expert-major already
    got = _exchange(engine, send, plan.send_counts, [list(row) for row in plan.matrix], operand)
    return _regroup(got, plan, inverse=False)


def dispatch_scaled(engine, x: torch.Tensor, plan: TokenPlan, row_scale: Optional[torch.Tensor], operand=None):
    """Dispatch ``x`` [T, ...] again along ``plan`` with every assignment's row times
    ``row_scale`` [T, K] (the combine's backward w.r.t. the expert rows): the route scatter with
    the plan's scan, clipping and matrix, no count exchange."""
    _check_rows("dispatchTokens", x)
    _check_plan_rows("dispatchTokens", x, plan, plan.num_tokens)
    row_scale = _check_weights(row_scale, plan, x)
    send, _ = _route_rows(x, plan._route, plan.top_k, sum(plan.send_counts), row_scale, plan._clip)
    return _forward_rows(engine, send, plan, operand)


# ---------------------------------------------------------------- combine
def _check_plan_rows(what: str, t: torch.Tensor, plan: TokenPlan, rows: int):
    if not isinstance(plan, TokenPlan):
        raise Mp4jException(f"{what}: plan must be the TokenPlan dispatchTokens returned")
    if t.shape[0] != rows:
        raise Mp4jException(f"{what}: {t.shape[0]} rows, the plan has {rows}")
    if tuple(t.shape[1:]) != plan.row_shape or t.dtype != plan.dtype or t.device != plan.slots.device:
        raise Mp4jException(f"{what}: rows {tuple(t.shape[1:])} {t.dtype} on {t.device} differ from the plan's "
                            f"{plan.row_shape} {plan.dtype} on {plan.slots.device}")


def _check_weights(weights, plan: TokenPlan, like: torch.Tensor):
    if weights is None:
        return None
    T, K = plan.num_tokens, plan.top_k
    ok = isinstance(weights, torch.Tensor) and weights.dtype == torch.float32 and weights.device == like.device and \
        (tuple(weights.shape) == (T, K) or (K == 1 and tuple(weights.shape) == (T,)))
    if not ok:
        raise Mp4jException(f"weights must be float32 [{T}, {K}] on {like.device}")
    return weights.contiguous()


def return_rows(engine, expert_rows: torch.Tensor, plan: TokenPlan, operand=None) -> torch.Tensor:
    """Expert rows back on their senders, in the sender's slot order."""
    if len(plan.matrix) == 1:
        return expert_rows
    back = _regroup(expert_rows, plan, inverse=True)
    p = len(plan.matrix)
    mat_t = [[plan.matrix[j][i] for j in range(p)] for i in range(p)]
    return _exchange(engine, back, plan.recv_counts, mat_t, operand)


def combine_local(back: torch.Tensor, plan: TokenPlan, weights: Optional[torch.Tensor]) -> torch.Tensor:
    T, K = plan.num_tokens, plan.top_k
    if _native_ok(back):
        from ..ops.device_ops import moe_combine
        return moe_combine(back, plan.slots, weights, T, K, max_slot=sum(plan.send_counts) - 1)
    return _torch_combine(back, plan.slots, weights, T, K)


def combine(engine, expert_rows: torch.Tensor, plan: TokenPlan, weights=None, operand=None, return_slot_rows=False):
    """``out`` [T, ...]: see ``ProcessCommSlave.combineTokens``."""
    if not isinstance(plan, TokenPlan):
        raise Mp4jException("combineTokens: plan must be the TokenPlan dispatchTokens returned")
    _check_rows("combineTokens", expert_rows)
    _check_plan_rows("combineTokens", expert_rows, plan, plan.num_rows)
    weights = _check_weights(weights, plan, expert_rows)
    back = return_rows(engine, expert_rows, plan, operand)
    out = combine_local(back, plan, weights)
    return (out, back) if return_slot_rows else out
