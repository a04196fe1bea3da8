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

Padded fixed-capacity layout (``source_capacity=S``): every source rank may send at most S rows to
every expert, its first S in assignment order, so every buffer of the step has a shape known before
the ids are seen and nothing leaves the device between the router and the combined output: no
count exchange, no host sync, and the pair can be recorded by ``DeviceEngine.capture``.

* send buffer ``[E*S, ...]``: the ``pe``-th of this rank's assignments with expert e sits in row
  ``e*S + pe`` iff ``pe < S`` (``slots[a]``, else -1); the rows ``[min(cnt[e], S), S)`` of every
  expert block are zeros.  Every row is written exactly once per call (the scatter, then a fill of
  the pad rows; no memset of the buffer).
* the exchange is the all-to-all with the constant count ``el*S`` (``el = E/p``): one copy plan on
  the IPC mesh that carries the rows and the ``kept`` counts together, else two equal-split
  ``all_to_all_single``.  Rank r returns ``rows [el, p*S, ...]``: ``rows[e, i*S + j]`` is source i's
  j-th kept row of expert ``r*el + e`` or zeros, and ``plan.valid[e, i]`` says how many are rows.
* the way back is the inverse regroup and the same fixed exchange, which lands ``[E*S, ...]`` in slot
  order; the combine reads it through ``slots`` and never reads a pad row.

A padded dispatch -> experts -> combine is, bit for bit, the uncapped call on the ids with every
assignment past its per-(rank, expert) share replaced by -1 (``tests/moe_padded_ref.py``).

Drop by gate weight (``priority=``, with any of the capacities above): where a rank must drop
assignments of an expert it keeps the ones with the largest ``(gate key of priority[a], -a)`` instead of
the first ones (:func:`priority_mask_torch` is the definition; K15, ``csrc/kernels/moe_priority.hip``, on
the GPU).  The ids with the losers set to -1 are counted again and take the position path, which then
has nothing left to drop: padded, the limit is the scalar S; ragged with a capacity, the limit is this
rank's quota ``keep[r]`` of the unchanged count exchange, so quotas between ranks stay in rank order and
the priority decides inside a rank.  The plan's route is the masked one and it has no clip table, so
every later combine and backward follows it unchanged.

The combine's backward (``combine_backward``, ``combineTokensBackward``) makes both of its gradients
from the output gradient ``g``: the expert rows' is ``g`` dispatched again along the plan with the
gate weights as row scale, the weights' the dot of ``g[t]`` with every slot row of token t.  Both
walk the same slots of buffers of one shape, so one pass does both (K11) and the exchange follows.

The layout of a plan is chosen in one place, :func:`_layout`, from ``source_capacity`` (by ``dispatch``
for a new plan, by ``TokenPlan`` for one built from keywords); the plan carries it as ``_layout``.  A
layout (:class:`_Ragged`, with or without a capacity, or :class:`_Padded`) answers what differs: how a
route becomes send rows and a plan (``route``); the K9 / K11 wrapper and the bound it is given
(``scatter``, ``combine``, ``combine_backward``); how rows cross ranks and change between source and
expert order (``exchange``, ``regroup``); the shape of the expert rows a combine takes
(``check_expert_rows``); whether the send buffer has rows nobody writes (``has_pad_rows``) and whether
a call may be captured (``capturable``).  Every torch form exists once and asks only ``has_pad_rows``.

GPU tensors run the K9 / K11 kernels (``csrc/kernels/moe.hip``); host tensors, and GPU tensors where
the native library is absent, run the torch implementation of the same contract below.
"""
from __future__ import annotations

import math
from itertools import accumulate
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
    dropped, ``sum_e demand_matrix[r][e] - expert_matrix[r][e]``.

    A padded call (``source_capacity`` = its S, else None) knows its shapes without the ids:
    ``expert_counts = (p*S,)*el``, ``send_counts = recv_counts = (el*S,)*p`` and ``matrix`` are
    constants, ``slots[a] = e*S + pe`` or -1.  What the ids decide stays on the device and is never
    read back by the library: ``kept`` int64 ``[E]`` (``min(cnt[e], S)`` on this rank), ``valid``
    int64 ``[el, p]`` (source i's kept rows of local expert e: ``rows[e, i*S : i*S + valid[e, i]]``
    are rows, the rest of the block zeros) and ``dropped`` int64 ``[3]`` (assignments past their
    share, negative ids, ids >= E).  ``clipped``, ``demand_matrix`` and ``expert_matrix`` are None
    there.  Inside a captured graph every replay rewrites ``slots``, ``kept``, ``valid``, ``dropped``."""
    __slots__ = ("num_tokens", "top_k", "num_experts", "expert_counts", "send_counts", "recv_counts", "slots",
                 "matrix", "expert_matrix", "row_shape", "dtype", "rank", "capacity", "demand_matrix", "clipped",
                 "source_capacity", "kept", "valid", "dropped", "_route", "_clip", "_layout", "_frozen")

    def __init__(self, **kw):
        kw = {"capacity": None, "demand_matrix": kw.get("expert_matrix"), "clipped": 0, "_clip": None,
              "source_capacity": None, "kept": None, "valid": None, "dropped": None, **kw}
        if "_layout" not in kw:
            kw["_layout"] = _layout(kw["source_capacity"])
        for k, v in kw.items():
            object.__setattr__(self, k, v)
        object.__setattr__(self, "_frozen", True)

    def __setattr__(self, name, value):
        raise AttributeError("TokenPlan is read-only")

    @property
    def num_rows(self) -> int:
        return sum(self.expert_counts)

    def segment_table(self):
        """The rows of every local expert as the table :func:`grouped_mm_torch` takes.  A
        padded plan: ``("padded", valid, S)``, the plan's own ``valid`` (rewritten by every replay of
        a captured dispatch).  A ragged plan: ``("ragged", offsets)``, int64 ``[E/p + 1]`` on the
        slots' device, the running sum of ``expert_counts``."""
        if self.source_capacity is not None:
            return ("padded", self.valid, self.source_capacity)
        offsets = [0] + list(accumulate(int(c) for c in self.expert_counts))
        return ("ragged", torch.tensor(offsets, dtype=torch.int64).to(self.slots.device))


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


def _check_rows(what: str, t: torch.Tensor, layout):
    if not isinstance(t, torch.Tensor):
        raise Mp4jException(f"{what} needs a torch tensor")
    if t.dim() < 1 or not t.is_contiguous():
        raise Mp4jException(f"{what}: rows must be a contiguous [rows, ...] tensor")
    if t.dtype not in DTYPES:
        raise Mp4jException(f"{what}: dtype {t.dtype} is not float32 / bfloat16 / float16")
    rb = _width(t.shape[1:]) * t.element_size()
    if rb == 0 or (t.is_cuda and rb % 16):
        raise Mp4jException(f"{what}: rows of {rb} bytes on a GPU tensor are not whole 16-byte vectors")
    if t.is_cuda and not layout.capturable:       # the padded layout exchanges no counts: it may be captured
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


def _torch_place(route, ids: torch.Tensor, nb: int, limit: torch.Tensor, base: torch.Tensor) -> torch.Tensor:
    """The slots of ``_torch_route``'s result under a per-expert limit: the ``pe``-th assignment of
    expert e (its position inside its expert, in assignment order) stays iff ``pe < limit[e]``, at
    slot ``base[e] + pe``; every other assignment gets -1."""
    counts, slots, order = route
    start = torch.cumsum(counts[:nb], 0) - counts[:nb]
    e = ids.to(torch.int64)[order]
    pe = torch.arange(order.numel(), dtype=torch.int64, device=ids.device) - start[e]
    stay = pe < limit[e]
    slots = torch.full_like(slots, -1)
    slots[order[stay]] = base[e[stay]] + pe[stay]
    return slots


def _torch_clip(route, ids: torch.Tensor, nb: int, keep: Sequence[int]) -> torch.Tensor:
    """The ragged slots under the quota ``keep[e]``: the kept assignments close ranks (still the
    stable sort), expert e's from ``kept_base[e]``, the exclusive prefix of ``keep``."""
    keep_t = torch.tensor(list(keep), dtype=torch.int64, device=ids.device)
    return _torch_place(route, ids, nb, keep_t, torch.cumsum(keep_t, 0) - keep_t)


def _torch_pad(route, ids: torch.Tensor, nb: int, S: int):
    """The torch form of the padded route: (slots int64[n], kept int64[nb], dropped int64[3]); expert
    e keeps its first S assignments, from slot ``e*S``."""
    counts = route[0]
    e = torch.arange(nb, dtype=torch.int64, device=ids.device)
    slots = _torch_place(route, ids, nb, torch.full_like(e, S), e * S)
    kept = counts[:nb].clamp(max=S)
    dropped = torch.stack([(counts[:nb] - kept).sum(), counts[nb], counts[nb + 1]])
    return slots, kept, dropped


def _torch_scatter(x: torch.Tensor, slots: torch.Tensor, top_k: int, row_scale: Optional[torch.Tensor],
                   out: torch.Tensor, has_pad_rows: bool) -> torch.Tensor:
    """``out[slots[a]] = x[a // K]`` (times ``row_scale[a]``, one rounding) for ``slots[a] >= 0``; the
    rows no slot names, which only a layout with pad rows has, are zeros."""
    if has_pad_rows:
        out.zero_()
    a = torch.nonzero(slots >= 0).reshape(-1)
    rows = x[a // top_k]
    if row_scale is not None:
        s = row_scale.reshape(-1)[a].view((-1,) + (1,) * (x.dim() - 1))
        rows = (s * rows.to(torch.float32)).to(x.dtype)
    out[slots[a]] = rows
    return out


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


def combine_weight_grad_torch(g: torch.Tensor, slots: torch.Tensor, slot_rows: torch.Tensor, T: int, K: int):
    """The combine's gradient w.r.t. its weights in torch, float32 ``[T, K]``: ``g_w[t, k] = g[t] .
    slot_rows[slots[t, k]]`` in float32, +0 where the slot is negative; zeros without rows or tokens."""
    if not (slot_rows.shape[0] and T):      # (a padded plan has rows even for a rank with no token)
        return torch.zeros((T, K), dtype=torch.float32, device=g.device)
    sl = slots.view(T, K)
    y = slot_rows.reshape(slot_rows.shape[0], -1)[sl.clamp(min=0)].to(torch.float32)      # [T, K, H]
    g_w = (g.reshape(T, 1, -1).to(torch.float32) * y).sum(-1)
    return torch.where(sl >= 0, g_w, torch.zeros_like(g_w))


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


# ---------------------------------------------------------------- drop by gate weight (K15)
def priority_mask_torch(ids: torch.Tensor, priority: torch.Tensor, nb: int, limit):
    """The definition of the per-expert top-S select in torch, and its CPU form: ``(out, masked)``.
    ``out[a] = ids[a]`` for the ``limit[e]`` assignments of every expert ``e = ids[a]`` in ``[0, nb)``
    with the largest ``(gate key of priority[a], -a)``, -1 for the expert's others; a negative id and
    an id ``>= nb`` pass through.  ``masked``: int64 ``[1]``, the assignments turned into -1.  ``limit``:
    an int or an int64 ``[nb]`` tensor (negative: 0).  The key comes from the float's bits by integer
    operations (unsigned order == float order, -0 folded onto +0, a positive NaN above +inf, a
    negative one below -inf) and the order from two stable sorts, by key descending and then by id: no
    float is ever compared."""
    flat = ids.reshape(-1)
    i64 = flat.to(torch.int64)
    n = i64.numel()
    bits = priority.reshape(-1).contiguous().view(torch.int32).to(torch.int64) & 0xffffffff
    bits = torch.where((bits & 0x7fffffff) == 0, torch.zeros_like(bits), bits)
    key = torch.where((bits >> 31) != 0, bits ^ 0xffffffff, bits ^ 0x80000000)
    placed = (i64 >= 0) & (i64 < nb)
    bucket = torch.where(placed, i64, torch.full_like(i64, nb))
    by_key = torch.argsort(0xffffffff - key, stable=True)               # equal keys: the lower a first
    order = by_key[torch.argsort(bucket[by_key], stable=True)]
    counts = torch.bincount(bucket, minlength=nb + 1)
    start = torch.cumsum(counts, 0) - counts
    if isinstance(limit, torch.Tensor):
        lim = limit.to(device=i64.device, dtype=torch.int64).reshape(-1)
    else:
        lim = torch.full((nb,), int(limit), dtype=torch.int64, device=i64.device)
    lim = torch.cat([lim, counts[nb:]])                                   # the bucket of the unplaced keeps all
    b = bucket[order]
    rank = torch.arange(n, dtype=torch.int64, device=i64.device) - start[b]
    gone = order[rank >= lim[b]]
    out = flat.clone()
    out[gone] = -1
    return out.view(ids.shape), torch.full((1,), gone.numel(), dtype=torch.int64, device=i64.device)


def _check_priority(priority, expert_ids: torch.Tensor, x: torch.Tensor, any_capacity: bool):
    """The caller's contract for ``priority``; returns it flattened, or None."""
    if priority is None:
        return None
    if not any_capacity:
        raise Mp4jException("dispatchTokens: priority needs capacity, capacityFactor or sourceCapacity: nothing is "
                            "dropped without one")
    T = expert_ids.shape[0]
    K = 1 if expert_ids.dim() == 1 else int(expert_ids.shape[1])
    ok = (isinstance(priority, torch.Tensor) and priority.dtype == torch.float32 and priority.device == x.device
          and (tuple(priority.shape) == (T, K) or (K == 1 and tuple(priority.shape) == (T,)))
          and priority.is_contiguous())
    if not ok:
        raise Mp4jException(f"dispatchTokens: priority must be a contiguous float32 [{T}, {K}] tensor on {x.device}")
    return priority.reshape(-1)


def _priority_route(x: torch.Tensor, ids: torch.Tensor, route, E: int, priority: torch.Tensor, limit):
    """The route of a priority call: the top ``limit[e]`` of every expert keep their id, the route is
    counted again on those ids, and everything behind it is the position path with nothing left to
    drop.  Returns (those ids, their route, masked int64 [1], the counts of the caller's ids); all on
    the device."""
    if _native_ok(x):
        from ..ops.device_ops import moe_priority_mask, moe_route_count
        ids_m, masked = moe_priority_mask(route, priority, limit)
        return ids_m, moe_route_count(ids_m, E), masked, route.counts
    ids_m, masked = priority_mask_torch(ids, priority, E, limit)
    return ids_m, _torch_route(ids_m, E), masked, route[0]


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
def _scatter(layout, x: torch.Tensor, route, top_k: int, row_scale: Optional[torch.Tensor], send: torch.Tensor,
             clip: Optional[torch.Tensor] = None):
    """Rows of ``x`` replicated into ``send`` along ``route`` (the second half of the route, times
    ``row_scale``); returns the slots.  ``route``: the native ``RouteCount``, in the torch form the slots.
    ``clip``: the device ``[keep | kept_base]`` of a capped native call (the torch form's slots are clipped
    already; a padded plan has none)."""
    if _native_ok(x):
        return layout.scatter(route, x, top_k, send, row_scale, clip)
    _torch_scatter(x, route, top_k, row_scale, send, layout.has_pad_rows)
    return route


def dispatch(engine, x: torch.Tensor, expert_ids: torch.Tensor, num_experts: int, operand=None, capacity=None,
             capacity_factor=None, source_capacity=None, priority=None):
    """``(rows, plan)``: see ``ProcessCommSlave.dispatchTokens``."""
    p = engine.p
    E = int(num_experts)
    _check_source_capacity(source_capacity, capacity, capacity_factor)
    layout = _layout(source_capacity)
    _check_rows("dispatchTokens", x, layout)
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
    priority = _check_priority(priority, expert_ids, x, source_capacity is not None or capacity is not None
                               or capacity_factor is not None)
    # the first half of the route: K9's histogram + scan, or its torch form
    if _native_ok(x):
        from ..ops.device_ops import moe_route_count
        route = moe_route_count(ids, E)
    else:
        route = _torch_route(ids, E)
    # the layout's: which counts cross ranks, the scatter, the exchange and what the plan says of them
    if priority is None:
        got, fields = layout.route(engine, x, ids, route, K, E, operand, capacity, capacity_factor)
    else:
        got, fields = layout.route(engine, x, ids, route, K, E, operand, capacity, capacity_factor, priority=priority)
    plan = TokenPlan(num_tokens=T, top_k=K, num_experts=E, row_shape=tuple(x.shape[1:]), dtype=x.dtype,
                     rank=engine.rank, source_capacity=source_capacity, _layout=layout, **fields)
    return layout.regroup(got, plan, inverse=False), plan


def _to_experts(engine, send: torch.Tensor, plan: TokenPlan, operand):
    """Send order to expert rows: the exchange, then the regroup."""
    layout = plan._layout
    return layout.regroup(layout.exchange(engine, send, plan, operand, back=False), plan, inverse=False)


def dispatch_scaled(engine, x: torch.Tensor, plan: TokenPlan, row_scale: Optional[torch.Tensor], operand=None):
    """Dispatch ``x`` [T, ...] again along ``plan`` with every assignment's row times
    ``row_scale`` [T, K] (the combine's backward w.r.t. the expert rows): the route scatter with
    the plan's scan, clipping and matrix, no count exchange."""
    _check_rows("dispatchTokens", x, plan._layout)
    _check_plan_rows("dispatchTokens", x, plan, plan.num_tokens)
    row_scale = _check_weights(row_scale, plan, x)
    send = torch.empty((sum(plan.send_counts),) + plan.row_shape, dtype=x.dtype, device=x.device)
    _scatter(plan._layout, x, plan._route, plan.top_k, row_scale, send, plan._clip)
    return _to_experts(engine, send, plan, operand)


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


def combine(engine, expert_rows: torch.Tensor, plan: TokenPlan, weights=None, operand=None, return_slot_rows=False):
    """``out`` [T, ...]: see ``ProcessCommSlave.combineTokens``."""
    if not isinstance(plan, TokenPlan):
        raise Mp4jException("combineTokens: plan must be the TokenPlan dispatchTokens returned")
    layout = plan._layout
    layout.check_expert_rows(expert_rows, plan)
    weights = _check_weights(weights, plan, expert_rows)
    # expert rows back on their senders, in the sender's slot order: the inverse regroup, then the exchange
    back = layout.exchange(engine, layout.regroup(expert_rows, plan, inverse=True), plan, operand, back=True)
    if _native_ok(back):
        out = layout.combine(back, plan, weights)
    else:
        out = _torch_combine(back, plan.slots, weights, plan.num_tokens, plan.top_k)
    return (out, back) if return_slot_rows else out


# ---------------------------------------------------------------- the combine's backward (K11)
COMBINE_BWD_MAX_TOP_K = 16      # csrc/kernels/moe.hip: kMoeBwdMaxK; a larger K runs the torch form


def _torch_combine_backward(g: torch.Tensor, plan: TokenPlan, weights: torch.Tensor, slot_rows: torch.Tensor):
    """The torch form of K11's contract: (the gradient rows in slot order, g_weights float32 [T, K])."""
    send = _torch_scatter(g, plan.slots, plan.top_k, weights, torch.empty_like(slot_rows), plan._layout.has_pad_rows)
    return send, combine_weight_grad_torch(g, plan.slots, slot_rows, plan.num_tokens, plan.top_k)


def combine_backward(engine, g: torch.Tensor, plan: TokenPlan, weights: torch.Tensor, slot_rows: torch.Tensor,
                     operand=None):
    """``(g_expert_rows, g_weights)``: see ``ProcessCommSlave.combineTokensBackward``."""
    what = "combineTokensBackward"
    if not isinstance(plan, TokenPlan):
        raise Mp4jException(f"{what}: plan must be the TokenPlan dispatchTokens returned")
    _check_rows(what, g, plan._layout)
    _check_plan_rows(what, g, plan, plan.num_tokens)
    if weights is None:
        raise Mp4jException(f"{what}: weights are needed (without them the backward is dispatchTokens along the plan)")
    weights = _check_weights(weights, plan, g)
    if not isinstance(slot_rows, torch.Tensor) or slot_rows.dim() < 1 or not slot_rows.is_contiguous():
        raise Mp4jException(f"{what}: slotRows must be the contiguous rows combineTokens(returnSlotRows=True) returned")
    _check_plan_rows(f"{what}: slotRows", slot_rows, plan, sum(plan.send_counts))
    if _native_ok(g) and plan.top_k <= COMBINE_BWD_MAX_TOP_K:
        send, g_w = plan._layout.combine_backward(g, slot_rows, plan, weights)
    else:
        send, g_w = _torch_combine_backward(g, plan, weights, slot_rows)
    return _to_experts(engine, send, plan, operand), g_w.view_as(weights)


# ---------------------------------------------------------------- the grouped expert GEMM: its definition
GROUPED_MM_ACTS = (None, "relu")


def _table_segments(table, rows: torch.Tensor, G: int) -> List[List[Tuple[int, int]]]:
    """Per group the ``(first row, row count)`` segments it owns in ``rows`` flattened to
    ``[R, width]``; reads the table on the host (the torch form only)."""
    if not isinstance(table, tuple) or not table or table[0] not in ("ragged", "padded"):
        raise ValueError("segment table must be ('ragged', offsets) or ('padded', valid, S)")
    if table[0] == "ragged":
        if len(table) != 2 or rows.dim() != 2 or table[1].numel() != G + 1:
            raise ValueError(f"a ragged table is ('ragged', offsets [{G + 1}]) over rows [R, width]")
        R, prev, segs = rows.shape[0], 0, []
        for hi in table[1].tolist()[1:]:
            hi = max(prev, min(int(hi), R))
            segs.append([(prev, hi - prev)])
            prev = hi
        return segs
    if len(table) != 3 or table[1].dim() != 2 or table[1].shape[0] != G:
        raise ValueError(f"a padded table is ('padded', valid [{G}, B], S)")
    B, S = table[1].shape[1], table[2]
    if isinstance(S, bool) or not isinstance(S, int) or S < 1 or B < 1:
        raise ValueError(f"a padded table's share S {S!r} must be an int >= 1 and B >= 1")
    if rows.dim() != 3 or tuple(rows.shape[:2]) != (G, B * S):
        raise ValueError(f"rows along this padded table are [{G}, {B * S}, width], not {tuple(rows.shape)}")
    valid = table[1].tolist()
    return [[((g * B + b) * S, max(0, min(int(valid[g][b]), S))) for b in range(B)] for g in range(G)]


def grouped_mm_torch(x: torch.Tensor, w: torch.Tensor, table, bias: Optional[torch.Tensor] = None, act=None,
                     transpose_w: bool = False, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The definition of the grouped GEMM in torch (float32 on the exactly converted operands, one
    rounding): ``out[r] = act(x[r] @ W[g] + bias[g])`` for the rows r group g owns along ``table``,
    +0 where ``mask <= 0``, and +0 in every row nobody owns (those rows of ``x`` and ``mask`` are
    never read).  It reads the table on the host; a kernel for it must not."""
    if act not in GROUPED_MM_ACTS:
        raise ValueError(f"act {act!r} is not None or 'relu'")
    G = w.shape[0]
    N = w.shape[1] if transpose_w else w.shape[2]
    segs = _table_segments(table, x, G)
    xf = x.reshape(-1, x.shape[-1])
    out = torch.zeros((xf.shape[0], N), dtype=x.dtype, device=x.device)
    mf = None if mask is None else mask.reshape(-1, N)
    for g in range(G):
        wg = w[g].to(torch.float32)
        wg = wg.t() if transpose_w else wg
        for lo, n in segs[g]:
            if n == 0:
                continue
            v = xf[lo:lo + n].to(torch.float32) @ wg
            if bias is not None:
                v = v + bias[g].to(torch.float32)
            if act == "relu":
                v = torch.relu(v)
            if mf is not None:
                v = torch.where(mf[lo:lo + n].to(torch.float32) <= 0, torch.zeros_like(v), v)
            out[lo:lo + n] = v.to(x.dtype)
    return out.view(tuple(x.shape[:-1]) + (N,))


def grouped_mm_wgrad_torch(x: torch.Tensor, gy: torch.Tensor, table, want_bias: bool = True):
    """The definition of the grouped weight gradient in torch: ``(gw [G, Kd, N], gb [G, N] or None)``,
    ``gw[g] = sum_r x[r]^T gy[r]`` and ``gb[g] = sum_r gy[r]`` over the rows group g owns, float32 on
    the exactly converted operands, one rounding; +0 for a group without rows."""
    G = table[1].shape[0] - 1 if table[0] == "ragged" else table[1].shape[0]
    segs = _table_segments(table, x, G)
    Kd, N = x.shape[-1], gy.shape[-1]
    xf, gf = x.reshape(-1, Kd), gy.reshape(-1, N)
    gw = torch.zeros((G, Kd, N), dtype=torch.float32, device=x.device)
    gb = torch.zeros((G, N), dtype=torch.float32, device=x.device)
    for g in range(G):
        for lo, n in segs[g]:
            if n == 0:
                continue
            xs, gs = xf[lo:lo + n].to(torch.float32), gf[lo:lo + n].to(torch.float32)
            gw[g] += xs.t() @ gs
            gb[g] += gs.sum(0)
    return gw.to(x.dtype), (gb.to(x.dtype) if want_bias else None)


# ---------------------------------------------------------------- the gated expert activation: its definition
def _glu_segments(fn: str, pre: torch.Tensor, g_h: Optional[torch.Tensor], table) -> List[Tuple[int, int]]:
    """The ``(first row, row count)`` segments somebody owns in ``pre`` flattened to ``[R, 2N]``, after
    the checks a kernel's wrapper would make; reads the table on the host (the torch form only)."""
    for name, t in (("pre", pre), ("g_h", g_h)):
        if t is None and name != "pre":
            continue
        if not isinstance(t, torch.Tensor) or t.dtype not in DTYPES:
            raise ValueError(f"{fn}: {name} must be a float32 / bfloat16 / float16 tensor")
        if not t.is_contiguous():
            raise ValueError(f"{fn}: {name} must be contiguous")
        if t.dtype != pre.dtype or t.device != pre.device:
            raise ValueError(f"{fn}: {name} must have pre's dtype and device")
    if pre.dim() < 2 or pre.shape[-1] % 2:
        raise ValueError(f"{fn}: pre must be [..., 2N]; its last dimension {tuple(pre.shape)[-1:]} is odd or missing")
    if not isinstance(table, tuple) or not table or table[0] not in ("ragged", "padded"):
        raise ValueError(f"{fn}: table must be ('ragged', offsets) or ('padded', valid, S)")
    tt = table[1] if len(table) > 1 else None
    if not isinstance(tt, torch.Tensor) or tt.dtype != torch.int64 or tt.device != pre.device:
        raise ValueError(f"{fn}: table must hold an int64 tensor on pre's device")
    if table[0] == "ragged" and (tt.dim() != 1 or tt.numel() < 1):
        raise ValueError(f"{fn}: a ragged table is ('ragged', offsets [G + 1]) over pre [R, 2N]")
    G = tt.numel() - 1 if table[0] == "ragged" else tt.shape[0]
    try:
        segs = _table_segments(table, pre, G)
    except ValueError as e:
        raise ValueError(f"{fn}: pre / table: {e}") from None
    if g_h is not None and tuple(g_h.shape) != tuple(pre.shape[:-1]) + (pre.shape[-1] // 2,):
        raise ValueError(f"{fn}: g_h must be {list(pre.shape[:-1]) + [pre.shape[-1] // 2]}, not {list(g_h.shape)}")
    return [seg for group in segs for seg in group if seg[1] > 0]


def glu_torch(pre: torch.Tensor, table) -> torch.Tensor:
    """The definition of the gated (SwiGLU) expert activation in torch, and its CPU form: with ``gate
    = pre[..., :N]`` and ``up = pre[..., N:]``, ``h = (g / (1 + exp(-g))) * u`` in float32 on the
    exactly converted operands with one rounding, for the rows somebody owns along ``table``; +0 in
    every row nobody owns (those rows of ``pre`` are never read).  It reads the table on the host;
    a kernel for it must not."""
    segs = _glu_segments("glu_torch", pre, None, table)
    N = pre.shape[-1] // 2
    flat = pre.reshape(_width(pre.shape[:-1]), 2 * N)
    out = torch.zeros((flat.shape[0], N), dtype=pre.dtype, device=pre.device)
    for lo, n in segs:
        rows = flat[lo:lo + n].to(torch.float32)
        g, u = rows[:, :N], rows[:, N:]
        out[lo:lo + n] = ((g / (1.0 + torch.exp(-g))) * u).to(pre.dtype)
    return out.view(tuple(pre.shape[:-1]) + (N,))


def glu_backward_torch(pre: torch.Tensor, g_h: torch.Tensor, table) -> torch.Tensor:
    """The closed-form backward of :func:`glu_torch` from the saved ``pre``: with ``s = 1 / (1 +
    exp(-g))`` and ``sm = 1 / (1 + exp(g))`` (by that formula, never ``1 - s``), ``g_pre[..., :N] =
    (g_h * u) * (s * (1 + g * sm))`` and ``g_pre[..., N:] = g_h * (g / (1 + exp(-g)))``, each with one
    rounding; +0 in every row nobody owns, where neither ``pre`` nor ``g_h`` is read."""
    segs = _glu_segments("glu_backward_torch", pre, g_h, table)
    N = pre.shape[-1] // 2
    R = _width(pre.shape[:-1])
    flat, gf = pre.reshape(R, 2 * N), g_h.reshape(R, N)
    out = torch.zeros_like(flat)
    for lo, n in segs:
        rows, d = flat[lo:lo + n].to(torch.float32), gf[lo:lo + n].to(torch.float32)
        g, u = rows[:, :N], rows[:, N:]
        den = 1.0 + torch.exp(-g)
        s, sm = 1.0 / den, 1.0 / (1.0 + torch.exp(g))
        out[lo:lo + n, :N] = ((d * u) * (s * (1.0 + g * sm))).to(pre.dtype)
        out[lo:lo + n, N:] = (d * (g / den)).to(pre.dtype)
    return out.view(pre.shape)


# ---------------------------------------------------------------- the padded fixed-capacity layout
def _check_source_capacity(source_capacity, capacity, capacity_factor):
    """The caller's contract, the same on every rank: refused before any work."""
    if source_capacity is None:
        return
    if capacity is not None or capacity_factor is not None:
        raise Mp4jException("dispatchTokens: sourceCapacity excludes capacity / capacityFactor (both need the demand "
                            "matrix, which the padded layout never gathers)")
    S = source_capacity
    if isinstance(S, bool) or not isinstance(S, int) or S < 1:
        raise Mp4jException(f"dispatchTokens: sourceCapacity {S!r} is not an int >= 1")


def _pad_buffers(x: torch.Tensor, E: int, S: int, p: int):
    """(send rows ``[E*S, ...]``, the counts' wire int64 ``[p, el_pad]``, el_pad) of a padded dispatch.
    On a GPU both are views of ONE allocation, rows first: the copy plan stages them from one base
    address.  Every destination's counts start on a 16-byte boundary (el_pad = el rounded up to even)."""
    el = E // p
    el_pad = el + (el & 1)
    shape = (E * S,) + tuple(x.shape[1:])
    if not x.is_cuda:
        return torch.empty(shape, dtype=x.dtype), torch.empty((p, el_pad), dtype=torch.int64), el_pad
    nbytes = E * S * _width(x.shape[1:]) * x.element_size()             # a multiple of 16 (_check_rows)
    whole = torch.empty(nbytes + p * el_pad * 8, dtype=torch.uint8, device=x.device)
    return whole[:nbytes].view(x.dtype).view(shape), whole[nbytes:].view(torch.int64).view(p, el_pad), el_pad


def _pad_ipc_inst(engine, like: torch.Tensor, need_bytes: int):
    """The IPC instance that runs a padded exchange of ``need_bytes`` per rank as one copy plan, or
    None (two equal-split all-to-alls).  The padded path's own qualification, every condition
    rank-independent: the environment, the device kind, the mesh, the payload inside one staging
    instance, and inside a capture an instance with device epochs (``IpcAllreduce._vec_ok``'s rule)."""
    from . import sparse
    from ..ops.native import capturing_now
    if not (sparse._SPARSE_IPC and like.is_cuda and engine.p > 1 and getattr(engine, "ipc_enabled", False)
            and engine.coll.__class__.__name__ == "TorchColl" and engine.algo in ("", "auto", "ipc")):
        return None
    if engine.ipc() is None:
        return None
    inst = sparse._ipc_inst(engine, need_bytes)
    if inst is None or (capturing_now() and inst._epoch_dev is None):
        return None
    return inst


def _pad_exchange(engine, send: torch.Tensor, wire: Optional[torch.Tensor], el_pad, operand):
    """The all-to-all with the constant count: block j of ``send`` (``rows / p`` rows) goes to rank
    j, and so does row j of ``wire`` (int64 ``[p, el_pad]``, the kept counts) when given.  Returns
    (rows in source order, the received counts or None).  One stream, no host sync."""
    p, r = engine.p, engine.rank
    if p == 1:
        return send, wire
    from ..ops.native import capturing_now
    n = send.shape[0]
    shape = tuple(send.shape)
    if send.is_cuda and operand is not None and not capturing_now():
        # the caller's operand (a wire codec) is the exact all-to-all's business, as in the ragged call
        got, _ = engine.all_to_all_v(send, [n // p] * p, None, operand, mat=[[n // p] * p] * p)
        got_wire = None
        if wire is not None:
            got_wire = torch.empty_like(wire)
            engine.coll.all_to_all_single(got_wire, wire)
        return got, got_wire
    nbytes = send.numel() * send.element_size()
    cbytes = wire.numel() * 8 if wire is not None else 0
    inst = _pad_ipc_inst(engine, send, nbytes + cbytes)
    if inst is not None:
        # One copy plan.  The plan's barriers are per block: block b of a rank may pull only what
        # block b of the peer staged, so a pull must start where a stage item starts (the same
        # relative index on both sides).  Hence one stage item per destination's rows (the own
        # block never crosses the mesh: a local copy), and the counts as ONE region that every rank
        # pulls whole from every peer (p * el_pad numbers), taking its own row of it afterwards:
        # p stage items and 2p - 1 pulls for any p the mesh allows.
        if wire is not None and wire.data_ptr() != send.data_ptr() + nbytes:
            raise Mp4jException("padded exchange: the counts do not follow the rows (see _pad_buffers)")
        rv, mv, cv = nbytes // 16, nbytes // 16 // p, cbytes // 16
        out = torch.empty(nbytes + p * cbytes, dtype=torch.uint8, device=send.device)
        stage = [(j * mv, j * mv, mv, 0) for j in range(p) if j != r] + ([(rv, rv, cv, 0)] if cv else [])
        pulls = [(r * mv, j * mv, mv, j) for j in range(p) if j != r]
        if cv:
            pulls += [(rv, rv + j * cv, cv, j) for j in range(p)]
        inst._plan(stage, pulls, send.data_ptr(), out.data_ptr(), mv)
        engine._count("all_to_all_v.ipc.padded")
        got = out[:nbytes].view(send.dtype).view(shape)
        got[r * (n // p):(r + 1) * (n // p)].copy_(send[r * (n // p):(r + 1) * (n // p)])
        return got, (out[nbytes:].view(torch.int64).view(p, p, el_pad)[:, r] if wire is not None else None)
    # equal splits: RCCL (capturable) on GPU tensors, bytes over the host backend otherwise
    raw = send.reshape(p, -1).view(torch.uint8)
    got = torch.empty_like(raw)
    engine.coll.all_to_all_single(got, raw)
    got_wire = None
    if wire is not None:
        got_wire = torch.empty_like(wire)
        engine.coll.all_to_all_single(got_wire, wire.contiguous())
    return got.view(send.dtype).view(shape), got_wire


def _pad_regroup(rows: torch.Tensor, plan: TokenPlan, inverse: bool) -> torch.Tensor:
    """``[p, el, S] -> [el, p*S]`` (or back, to ``[E*S]`` rows): one fixed strided copy; with one
    local expert or one rank the two orders coincide and the result is a view."""
    p = len(plan.matrix)
    el, S = plan.num_experts // p, plan.source_capacity
    if el > 1 and p > 1:
        rows = rows.view(((el, p, S) if inverse else (p, el, S)) + plan.row_shape).transpose(0, 1).contiguous()
    return rows.view(((p * el * S,) if inverse else (el, p * S)) + plan.row_shape)


# ---------------------------------------------------------------- the two layouts
class _Ragged:
    """Packed send order: ``sum(send_counts)`` rows, each written by the scatter.  One count exchange
    makes the plan; the rows cross ranks by the ragged all-to-all with that matrix.  It holds no state: a
    capacity's clip table is the plan's."""
    has_pad_rows = capturable = False
    regroup = staticmethod(_regroup)

    def route(self, engine, x, ids, route, K, E, operand, capacity, capacity_factor, priority=None):
        p, r = engine.p, engine.rank
        native = _native_ok(x)
        counts = route.counts if native else route[0]
        # the one count exchange: E + 2 numbers per rank
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
            if native:                      # keep | its exclusive prefix: one small H2D copy
                kbase = [0] + list(accumulate(keep))[:-1]
                clip = torch.tensor(list(keep) + kbase, dtype=torch.int64).to(x.device)
        if priority is not None:
            # drop by gate weight: the quota keep[e] is the position call's (between ranks the capacity
            # is still handed out in rank order); inside this rank the top keep[e] of expert e stay.
            # The plan's route is the one of the masked ids and nothing is left to clip
            limit = clip[:E] if native else torch.tensor(list(emat[r]), dtype=torch.int64)
            route = _priority_route(x, ids, route, E, priority, limit)[1]
            clip = None
            if not native:
                route = route[1]
        elif not native:                    # the torch form's route is its slots, clipped here
            route = route[1] if C is None else _torch_clip(route, ids, E, emat[r])
        el = E // p
        mat = tuple(tuple(sum(emat[i][j * el:(j + 1) * el]) for j in range(p)) for i in range(p))
        send_counts = mat[r]
        send = torch.empty((sum(send_counts),) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
        slots = _scatter(self, x, route, K, None, send, clip)
        got = self._a2a(engine, send, send_counts, mat, operand)
        return got, dict(expert_counts=tuple(sum(emat[i][r * el + e] for i in range(p)) for e in range(el)),
                         send_counts=send_counts, recv_counts=tuple(mat[i][r] for i in range(p)), slots=slots,
                         matrix=mat, expert_matrix=emat, capacity=C, demand_matrix=demand, clipped=clipped,
                         _route=route, _clip=clip)

    def scatter(self, route, x, top_k, send, row_scale, clip):
        from ..ops.device_ops import moe_route_scatter
        return moe_route_scatter(route, x, top_k, send, row_scale=row_scale, placed=send.shape[0], clip=clip)

    @staticmethod
    def _a2a(engine, rows, counts, mat, operand):
        if len(counts) == 1:
            return rows                     # one rank: send order is expert-major already
        return _exchange(engine, rows, counts, [list(row) for row in mat], operand)

    def exchange(self, engine, rows, plan, operand, back):
        if back:                            # the transposed matrix lands rows in the sender's slot order
            return self._a2a(engine, rows, plan.recv_counts, zip(*plan.matrix), operand)
        return self._a2a(engine, rows, plan.send_counts, plan.matrix, operand)

    def check_expert_rows(self, rows, plan):
        _check_rows("combineTokens", rows, self)
        if rows.dim() >= 2 and tuple(rows.shape[2:]) == plan.row_shape and tuple(rows.shape[1:]) != plan.row_shape:
            raise Mp4jException(f"combineTokens: rows {tuple(rows.shape)} are in the padded [experts, rows, ...] "
                                f"layout, the plan is a ragged one (no sourceCapacity)")
        _check_plan_rows("combineTokens", rows, plan, plan.num_rows)

    def combine(self, back, plan, weights):
        from ..ops.device_ops import moe_combine
        return moe_combine(back, plan.slots, weights, plan.num_tokens, plan.top_k, max_slot=sum(plan.send_counts) - 1)

    def combine_backward(self, g, slot_rows, plan, weights):
        from ..ops.device_ops import moe_combine_backward
        return moe_combine_backward(g, slot_rows, plan.slots, weights, plan.num_tokens, plan.top_k,
                                    max_slot=sum(plan.send_counts) - 1)


class _Padded:
    """``E*S`` send rows, expert e's block at ``e*S``, the rows behind its kept ones zeros.  Every shape
    is known before the ids are: no count exchange, nothing read back, nothing copied to the device."""
    has_pad_rows = capturable = True
    regroup = staticmethod(_pad_regroup)

    def __init__(self, S: int):
        self.S = S

    def route(self, engine, x, ids, route, K, E, operand, *_no_capacity, priority=None):
        p, S = engine.p, self.S
        el = E // p
        engine._count("moe.dispatch.padded")
        send, wire, el_pad = _pad_buffers(x, E, S, p)
        masked = None
        if priority is not None:            # drop by gate weight: the top S of every expert, then the position path
            ids, route, masked, counts = _priority_route(x, ids, route, E, priority, S)
        if _native_ok(x):
            from ..ops.device_ops import moe_pad_counts
            _, dropped = moe_pad_counts(route, S, group=el, group_pad=el_pad, kept=wire.view(-1))
        else:
            route, kept, dropped = _torch_pad(route, ids, E, S)
            wire.zero_()
            wire[:, :el] = kept.view(p, el)
        if masked is not None:
            # `dropped` keeps its meaning: past the share | negative | >= E, of the caller's ids (the
            # masked route has nothing past its share and counts the masked ones as negative)
            dropped = torch.cat([masked, counts[E:E + 2]])
        slots = _scatter(self, x, route, K, None, send)
        got, got_wire = _pad_exchange(engine, send, wire, el_pad, operand)
        const = (el * S,) * p
        return got, dict(expert_counts=(p * S,) * el, send_counts=const, recv_counts=const, slots=slots,
                         matrix=(const,) * p, expert_matrix=None, demand_matrix=None, clipped=None,
                         kept=wire[:, :el].reshape(E), valid=got_wire[:, :el].t().contiguous(), dropped=dropped,
                         _route=route)

    def scatter(self, route, x, top_k, send, row_scale, _no_clip=None):
        from ..ops.device_ops import moe_route_scatter_pad
        return moe_route_scatter_pad(route, x, top_k, send, self.S, row_scale=row_scale)

    def exchange(self, engine, rows, plan, operand, back):
        return _pad_exchange(engine, rows, None, None, operand)[0]        # the same fixed exchange both ways

    def check_expert_rows(self, rows, plan):
        p = len(plan.matrix)
        want = (plan.num_experts // p, p * self.S) + plan.row_shape
        if not isinstance(rows, torch.Tensor) or tuple(rows.shape) != want:
            raise Mp4jException(f"combineTokens: the plan is a padded one (sourceCapacity {self.S}): rows must be "
                                f"{want}, not {tuple(getattr(rows, 'shape', ()))}")
        if not rows.is_contiguous() or rows.dtype != plan.dtype or rows.device != plan.slots.device:
            raise Mp4jException(f"combineTokens: rows must be contiguous {plan.dtype} on {plan.slots.device}")

    def combine(self, back, plan, weights):
        from ..ops.device_ops import moe_combine_rows
        return moe_combine_rows(back, plan.slots, weights, plan.num_tokens, plan.top_k)

    def combine_backward(self, g, slot_rows, plan, weights):
        from ..ops.device_ops import moe_combine_backward
        return moe_combine_backward(g, slot_rows, plan.slots, weights, plan.num_tokens, plan.top_k,
                                    pad=(plan._route, self.S))


def _layout(source_capacity):
    """The layout of a plan, chosen here and nowhere else: padded iff there is a per-source share."""
    return _Ragged() if source_capacity is None else _Padded(source_capacity)

