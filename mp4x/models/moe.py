"""Expert-parallel mixture-of-experts layer on ``dispatchTokens`` / ``combineTokens``.

Rank ``r`` of ``p`` holds experts ``[r*E/p, (r+1)*E/p)``; every rank routes its own tokens.  The
two collectives are differentiable here:

* :func:`dispatch_tokens` — backward is a combine with unit weights on the return path: the
  gradient of token t is the sum, in k order, of the gradients of its K dispatched rows;
* :func:`combine_tokens` — backward w.r.t. the expert rows is a dispatch of the output gradient
  along the same plan with every assignment's row scaled by its gate weight (the K9 route scatter
  with ``row_scale``; the plan's count matrix, no new count exchange); backward w.r.t. the weights
  is the row dot ``sum_h g[t, h] * y[slot(t, k), h]`` in torch (not a hot path here).

Both backward passes are collectives: every rank must run them, in the same order, which autograd
does for the same graph on every rank.

:class:`ExpertParallelMoE` is the layer: router linear -> softmax -> top-k -> dispatch -> each
local expert's two-layer MLP on its ``expert_counts`` slice -> combine with the gate weights.

With an expert capacity (``capacity`` / ``capacity_factor``, see ``dispatchTokens``) the assignments
past an expert's first C are clipped inside the dispatch: their slots are -1 in the plan, so both
backward passes leave them out exactly as the forward did.

With a per-source share (``source_capacity=S``, the padded fixed-capacity layout of
``dispatchTokens``) the dispatched rows are ``[local experts, p*S, d]`` with zero rows behind every
source's kept rows, and the layer's experts run as two batched GEMMs over that tensor.  Both backward
passes follow the plan: the dispatch's is the unit-weight combine (pad rows are never read), the
combine's is the padded scatter with the gate weights as ``row_scale`` (pad rows of the gradient are
zero, so they add exactly zero to every expert-weight gradient).  Forward only can be captured
(``comm.device.capture``); capturing autograd is out of scope.
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional

import torch

from ..operands import Operands
from ..operators import Operators
from ..parallel.moe import combine_weight_grad_torch


class _Dispatch(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, comm, expert_ids, num_experts, operand, capacity, capacity_factor, source_capacity,
                priority=None):
        extra = {} if priority is None else {"priority": priority}      # (None: the call as it always was)
        rows, plan = comm.dispatchTokens(x.contiguous(), expert_ids, num_experts, operand=operand, capacity=capacity,
                                         capacityFactor=capacity_factor, sourceCapacity=source_capacity, **extra)
        ctx.comm, ctx.plan, ctx.operand = comm, plan, operand
        return rows, plan

    @staticmethod
    def backward(ctx, g_rows, _plan=None):
        gx = ctx.comm.combineTokens(g_rows.contiguous(), ctx.plan, None, operand=ctx.operand)
        return gx, None, None, None, None, None, None, None, None


class _Combine(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rows, weights, comm, plan, operand, backward="torch"):
        out, back = comm.combineTokens(rows.contiguous(), plan, weights, operand=operand, returnSlotRows=True)
        ctx.comm, ctx.plan, ctx.operand, ctx.fused = comm, plan, operand, backward == "fused"
        ctx.save_for_backward(back, weights)
        return out

    @staticmethod
    def backward(ctx, g):
        back, weights = ctx.saved_tensors
        plan = ctx.plan
        g = g.contiguous()
        if ctx.fused and weights is not None:
            g_rows, g_w = ctx.comm.combineTokensBackward(g, plan, weights, back, operand=ctx.operand)
            return g_rows, (g_w if ctx.needs_input_grad[1] else None), None, None, None, None
        g_rows, _ = ctx.comm.device.dispatch_tokens(g, None, plan.num_experts, ctx.operand, plan=plan,
                                                    row_scale=weights)
        g_w = None
        if weights is not None and ctx.needs_input_grad[1]:
            g_w = combine_weight_grad_torch(g, plan.slots, back, plan.num_tokens, plan.top_k).view_as(weights)
        return g_rows, g_w, None, None, None, None


def dispatch_tokens(comm, x: torch.Tensor, expert_ids: torch.Tensor, num_experts: int, operand=None, capacity=None,
                    capacity_factor=None, source_capacity=None, priority=None):
    """Differentiable ``comm.dispatchTokens``: ``(rows, plan)``.  With an expert capacity, or a
    per-source share (``source_capacity``: the padded layout, ``rows`` ``[E/p, p*S, ...]``), a
    clipped assignment has slot -1 in the plan: it takes no part in either backward pass (no
    gradient reaches its token through it, and its gate weight's gradient is 0).  ``priority``
    (float32 ``[T, K]``, see ``dispatchTokens``) only chooses which assignments those are: it is not
    differentiated."""
    if priority is None:
        return _Dispatch.apply(x, comm, expert_ids, num_experts, operand, capacity, capacity_factor, source_capacity)
    return _Dispatch.apply(x, comm, expert_ids, num_experts, operand, capacity, capacity_factor, source_capacity,
                           priority.detach())


COMBINE_BACKWARDS = ("torch", "fused")


def combine_tokens(comm, expert_rows: torch.Tensor, plan, weights: Optional[torch.Tensor] = None, operand=None,
                   backward: str = "torch"):
    """Differentiable ``comm.combineTokens`` (w.r.t. the rows and the weights).  ``backward="fused"``
    takes both gradients from ``comm.combineTokensBackward`` when ``weights`` are given (the rows'
    gradient has the same bits, the weights' is summed in another order); ``"torch"`` is the
    dispatch with ``row_scale`` and the row dots in torch."""
    if backward not in COMBINE_BACKWARDS:
        raise ValueError(f"backward {backward!r} is not 'torch' or 'fused'")
    return _Combine.apply(expert_rows, weights, comm, plan, operand, backward)


# ---------------------------------------------------------------- the router gate (K10)
GATE_MAX_EXPERTS, GATE_MAX_TOP_K = 2048, 16      # csrc/kernels/moe_gate.hip: kGateMaxE, kGateMaxK


class GateResult(NamedTuple):
    """What :func:`route_topk` returns.  ``weights`` float32 [T, K], ``lse`` float32 [T] and
    ``prob_sum`` float32 [E] are differentiable; ``ids`` [T, K] and ``counts`` int64 [E] are not.
    ``prob_sum`` and ``counts`` are None without ``stats``."""
    weights: torch.Tensor
    ids: torch.Tensor
    lse: torch.Tensor
    prob_sum: Optional[torch.Tensor]
    counts: Optional[torch.Tensor]


def _sum_in_k_order(q: torch.Tensor) -> torch.Tensor:
    s = q[:, 0]
    for k in range(1, q.shape[1]):
        s = s + q[:, k]
    return s


def gate_forward_torch(logits: torch.Tensor, top_k: int, renormalize: bool, ids_dtype, stats: bool):
    """The definition of the gate in torch (float32 on the exactly converted logits): what K10
    computes, for host tensors and for shapes outside the kernel's range.  It is the group-limited
    definition with the softmax score, no bias, one group and scale 1, bit for bit."""
    return gate_group_forward_torch(logits, top_k, "softmax", None, 1, 1, renormalize, 1.0, ids_dtype, stats)[:5]


def gate_backward_torch(logits: torch.Tensor, lse: torch.Tensor, ids: torch.Tensor, renormalize: bool,
                        g_weights: Optional[torch.Tensor], g_lse: Optional[torch.Tensor],
                        g_prob_sum: Optional[torch.Tensor]) -> torch.Tensor:
    """The closed-form backward of the gate in torch, from the saved logits, lse and ids; an absent
    gradient counts as zero.  One rounding to the logits' dtype."""
    return gate_group_backward_torch(logits, lse, ids, "softmax", renormalize, 1.0, g_weights, g_lse, g_prob_sum)


def _gate_is_fused(logits: torch.Tensor, top_k: int) -> bool:
    return (logits.is_cuda and logits.dtype in (torch.float32, torch.bfloat16, torch.float16)
            and 1 <= logits.shape[1] <= GATE_MAX_EXPERTS and top_k <= GATE_MAX_TOP_K)


def route_topk(logits: torch.Tensor, top_k: int, renormalize: bool = False, ids_dtype=torch.int64,
               stats: bool = False) -> GateResult:
    """The router gate over ``logits`` [T, E], differentiable: softmax, the top K experts of every
    token in the order (logit descending, expert index ascending; ``-inf`` is a mask), their
    probabilities as gate weights (``renormalize``: divided by their sum), the row log-sum-exp and,
    with ``stats``, ``prob_sum[e] = sum_t p[t, e]`` and ``counts[e]`` = tokens routed to e.

    On a GPU tensor with ``E <= 2048`` and ``top_k <= 16`` forward and backward are the fused K10
    kernels (one pass over the logits each, no host synchronisation, bit-reproducible); anywhere
    else they are the same definition in torch."""
    if logits.dim() != 2 or not logits.is_floating_point():
        raise ValueError("route_topk: logits must be a floating-point [T, E] tensor")
    if isinstance(top_k, bool) or not isinstance(top_k, int) or not 1 <= top_k <= logits.shape[1]:
        raise ValueError(f"route_topk: top_k {top_k!r} is not an int in [1, E = {logits.shape[1]}]")
    if ids_dtype not in (torch.int32, torch.int64):
        raise ValueError("route_topk: ids_dtype must be int32 or int64")
    return GateResult(*_RouteTopK.apply(logits, None, top_k, "softmax", 1, 1, bool(renormalize), 1.0, ids_dtype, bool(stats),
                                        False)[:5])


# ---------------------------------------------------------------- the group-limited router gate (K13)
GATE_MAX_GROUPS = 32                              # csrc/kernels/moe_gate_group.hip: kGateMaxGroups
GATE_SCORES = ("softmax", "sigmoid")


class GroupedGateResult(NamedTuple):
    """What :func:`route_topk_grouped` returns.  ``weights`` float32 [T, K], ``lse`` float32 [T]
    (None for the sigmoid score) and ``prob_sum`` float32 [E] are differentiable; ``ids`` [T, K],
    ``counts`` int64 [E] and ``group_ids`` int32 [T, topk_group] are not.  ``prob_sum`` and
    ``counts`` are None without ``stats``."""
    weights: torch.Tensor
    ids: torch.Tensor
    lse: Optional[torch.Tensor]
    prob_sum: Optional[torch.Tensor]
    counts: Optional[torch.Tensor]
    group_ids: torch.Tensor


def _sigmoid(x: torch.Tensor) -> torch.Tensor:
    return 1.0 / (1.0 + torch.exp(-x))


def gate_group_forward_torch(logits: torch.Tensor, top_k: int, score: str, bias: Optional[torch.Tensor], n_group: int,
                             topk_group: int, renormalize: bool, scale: float, ids_dtype, stats: bool):
    """The definition of the group-limited gate in torch (float32 on the exactly converted logits):
    what K13 computes, for host tensors and for shapes outside the kernel's range.
    ``(weights, ids, lse, prob_sum, counts, group_ids)``."""
    lg = logits.to(torch.float32)
    T, E = lg.shape
    n = E // n_group
    lse = None
    if score == "softmax":
        m = lg.max(dim=-1, keepdim=True).values if T else lg.new_zeros((0, 1))
        ex = torch.exp(lg - m)
        total = ex.sum(dim=-1, keepdim=True)
        lse = (m + torch.log(total)).squeeze(-1)
        s = ex / total
    else:
        s = _sigmoid(lg)
    neg = torch.full_like(s, float("-inf"))
    c = torch.where(lg == float("-inf"), neg, s if bias is None else s + bias.to(torch.float32))
    # a group's score: its two largest selection scores in one addition, the largest alone when the
    # second is -inf (one live column, or a group of one)
    top = c.view(T, n_group, n).topk(min(2, n), dim=-1).values
    gs = top[..., 0]
    if n > 1:
        gs = torch.where(top[..., 1] == float("-inf"), top[..., 0], top[..., 0] + top[..., 1])
    # (group score descending, group index ascending): the stable sort keeps equal scores in index order
    group_ids = torch.sort(gs, dim=-1, descending=True, stable=True).indices[:, :topk_group]
    inside = torch.zeros(T, n_group, dtype=torch.bool, device=lg.device).scatter_(1, group_ids, True)
    inside = inside.repeat_interleave(n, dim=1)
    # (key descending, index ascending) over the columns of the chosen groups: the key is the logit
    # without a bias, the selection score with one; a second stable sort moves the other groups' columns behind
    order = torch.sort(lg if bias is None else c, dim=-1, descending=True, stable=True).indices
    keep = torch.sort(inside.gather(1, order).to(torch.int8), dim=-1, descending=True, stable=True).indices
    ids = order.gather(1, keep)[:, :top_k]
    w = s.gather(1, ids)
    if renormalize:
        w = w / _sum_in_k_order(w).unsqueeze(1)
    w = w * scale
    prob_sum = counts = None
    if stats:
        prob_sum = s.sum(dim=0)
        counts = torch.bincount(ids.reshape(-1), minlength=E)
    return w, ids.to(ids_dtype), lse, prob_sum, counts, group_ids.to(torch.int32)


def gate_group_backward_torch(logits: torch.Tensor, lse: Optional[torch.Tensor], ids: torch.Tensor, score: str,
                              renormalize: bool, scale: float, g_weights: Optional[torch.Tensor],
                              g_lse: Optional[torch.Tensor], g_prob_sum: Optional[torch.Tensor]) -> torch.Tensor:
    """The closed-form backward of the group-limited gate in torch, from the saved logits, ids and
    (softmax) lse; an absent gradient counts as zero; the bias has no gradient.  One rounding to the
    logits' dtype."""
    lg = logits.to(torch.float32)
    ids = ids.to(torch.int64)
    p = torch.exp(lg - lse.unsqueeze(1)) if score == "softmax" else _sigmoid(lg)
    gp = torch.zeros_like(p) if g_prob_sum is None else g_prob_sum.unsqueeze(0).expand_as(p).clone()
    if g_weights is not None:
        gq = g_weights
        if renormalize:
            q = p.gather(1, ids)
            s = _sum_in_k_order(q).unsqueeze(1)
            gq = (g_weights - _sum_in_k_order(g_weights * (q / s)).unsqueeze(1)) / s
        gp.scatter_add_(1, ids, gq * scale)
    if score == "softmax":
        dot = (gp * p).sum(dim=-1, keepdim=True)
        g = p * (gp - dot)
        if g_lse is not None:
            g = g + g_lse.unsqueeze(1) * p
    else:
        g = (p * _sigmoid(-lg)) * gp              # sigmoid(l) * sigmoid(-l): never 1 - s
    return g.to(logits.dtype)


def _gate_group_is_fused(logits: torch.Tensor, top_k: int, n_group: int) -> bool:
    return _gate_is_fused(logits, top_k) and n_group <= GATE_MAX_GROUPS


class _RouteTopK(torch.autograd.Function):
    """Both gates.  ``grouped`` says which device ops a GPU tensor goes to: K13's for
    :func:`route_topk_grouped`, K10's (no score or group pass: the faster forward) for :func:`route_topk`,
    which passes the softmax score, no bias, one group and scale 1.  Anywhere else it is the one
    definition in torch."""

    @staticmethod
    def forward(ctx, logits, bias, top_k, score, n_group, topk_group, renormalize, scale, ids_dtype, stats, grouped):
        logits = logits.contiguous()
        ctx.fused = _gate_group_is_fused(logits, top_k, n_group) if grouped else _gate_is_fused(logits, top_k)
        if not ctx.fused:
            out = gate_group_forward_torch(logits, top_k, score, bias, n_group, topk_group, renormalize, scale, ids_dtype,
                                           stats)
        else:
            from ..ops import device_ops
            if grouped:
                out = device_ops.moe_gate_group_topk(logits, top_k, score, bias, n_group, topk_group, renormalize, scale,
                                                     ids_dtype, stats)
            else:
                out = device_ops.moe_gate_topk(logits, top_k, renormalize, ids_dtype, stats) + (None,)
        w, ids, lse, prob_sum, counts, group_ids = out
        ctx.score, ctx.renormalize, ctx.scale, ctx.grouped = score, renormalize, scale, grouped
        ctx.save_for_backward(logits, lse, ids)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(*(t for t in (ids, counts, group_ids) if t is not None))
        return w, ids, lse, prob_sum, counts, group_ids

    @staticmethod
    def backward(ctx, g_w, _g_ids, g_lse, g_psum, _g_counts, _g_groups):
        logits, lse, ids = ctx.saved_tensors
        g_w, g_lse, g_psum = (None if g is None else g.to(torch.float32).contiguous() for g in (g_w, g_lse, g_psum))
        if not ctx.fused:
            g = gate_group_backward_torch(logits, lse, ids, ctx.score, ctx.renormalize, ctx.scale, g_w, g_lse, g_psum)
        else:
            from ..ops import device_ops
            if ctx.grouped:
                g = device_ops.moe_gate_group_backward(logits, lse, ids, ctx.score, ctx.renormalize, ctx.scale, g_w, g_lse,
                                                       g_psum)
            else:
                g = device_ops.moe_gate_backward(logits, lse, ids, ctx.renormalize, g_w, g_lse, g_psum)
        return (g,) + (None,) * 10




def route_topk_grouped(logits: torch.Tensor, top_k: int, *, score: str = "sigmoid", bias: Optional[torch.Tensor] = None,
                       n_group: int = 1, topk_group: Optional[int] = None, renormalize: bool = False, scale: float = 1.0,
                       ids_dtype=torch.int64, stats: bool = False) -> GroupedGateResult:
    """The group-limited, bias-corrected router gate over ``logits`` [T, E], differentiable in the
    logits (the bias steers the selection only and has no gradient).

    The score s is the softmax over the experts or ``1 / (1 + exp(-l))``.  The selection score is
    ``s + bias`` (``bias`` float32 [E]; ``-inf`` logits are a mask).  The E experts form ``n_group``
    contiguous groups; a token takes the ``topk_group`` groups with the largest sum of their two
    largest selection scores (ties to the smaller group index; ``group_ids``), then the first K
    experts inside them in the order (selection score descending, expert index ascending; without a
    bias the logits' own order, which is :func:`route_topk`'s for any bits).  The gate weights are
    the chosen s, with ``renormalize`` divided by their sum, times ``scale``.  ``lse`` exists for the
    softmax score only.  With ``stats``: ``prob_sum[e] = sum_t s[t, e]`` and ``counts[e]``.

    On a GPU tensor with ``E <= 2048``, ``top_k <= 16`` and ``n_group <= 32`` forward and backward are
    the fused K13 kernels (no host synchronisation, bit-reproducible); anywhere else they are the
    same definition in torch."""
    from ..ops.device_ops import gate_group_args
    fn = "route_topk_grouped"
    if logits.dim() != 2 or not logits.is_floating_point():
        raise ValueError(f"{fn}: logits must be a floating-point [T, E] tensor")
    E = logits.shape[1]
    if isinstance(top_k, bool) or not isinstance(top_k, int) or not 1 <= top_k <= E:
        raise ValueError(f"{fn}: top_k {top_k!r} is not an int in [1, E = {E}]")
    n_group, topk_group, scale = gate_group_args(f"{fn}: ", E, top_k, score, n_group, topk_group, scale)
    if bias is not None:
        if (not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32 or tuple(bias.shape) != (E,)
                or bias.device != logits.device):
            raise ValueError(f"{fn}: bias must be a float32 [{E}] tensor on the logits' device")
        bias = bias.detach().contiguous()
    if ids_dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{fn}: ids_dtype must be int32 or int64")
    return GroupedGateResult(*_RouteTopK.apply(logits, bias, top_k, score, n_group, topk_group, bool(renormalize), scale,
                                               ids_dtype, bool(stats), True))


DROP_POLICIES = ("position", "probs")


class ExpertParallelMoE(torch.nn.Module):
    """Top-k routed mixture of two-layer ReLU MLP experts, experts sharded over the ranks.

    The full parameter set is drawn from ``seed`` on every rank (:meth:`init_weights`) and this rank
    keeps the router (replicated) and its own experts' slices, so a single-process model built from
    the same seed holds exactly the same weights.  After ``backward`` call :meth:`sync_gradients`:
    for a loss that is the mean over ranks of per-rank losses it averages the router's gradient
    over the ranks and scales the experts' (already summed over every rank's tokens by the
    combine / dispatch backward) by ``1/p``.

    ``capacity_factor``: every expert accepts the first ``max(1, ceil(f * N / E))`` of the step's N
    assignments (all ranks') in (rank, token, k) order; the others are dropped (``dispatchTokens``).
    ``last_plan`` is the last forward's plan (``clipped``, ``demand_matrix``), None before it.

    ``source_capacity`` (excludes ``capacity_factor``): every rank sends at most S of its
    assignments to every expert, its first in (token, k) order, in the padded layout of
    ``dispatchTokens(sourceCapacity=S)``: no host synchronisation in the step, and the local experts
    run as two batched GEMMs (``baddbmm`` over ``[local experts, p*S, d_model]``, ReLU between them)
    instead of a ragged loop.  ``last_plan.kept`` / ``valid`` / ``dropped`` stay on the device.

    ``router="fused"`` routes through :func:`route_topk` (the K10 kernels on the GPU) instead of
    :meth:`route`: a specified tie order, ``renormalize`` (gate weights divided by their sum over
    the chosen K) and the router's auxiliary losses.  Every forward then stores ``last_aux_loss``,
    over this rank's own tokens and with no collective, for the user to add to the loss:
    ``aux_loss_coef * E * sum_e (counts[e] / (T*K)) * (prob_sum[e] / T) + z_loss_coef * mean_t
    lse[t]^2``.  The default ``router="torch"`` is the layer as it was.

    ``score``, ``expert_groups``, ``topk_groups``, ``routed_scale`` and ``balance_bias`` (all need
    ``router="fused"``) route through :func:`route_topk_grouped` (the K13 kernels on the GPU):
    ``score="sigmoid"`` scores every expert on its own (no ``lse``: ``z_loss_coef`` is refused);
    ``expert_groups=Gr`` splits the experts into Gr contiguous groups of which a token uses
    ``topk_groups``; ``routed_scale`` multiplies the gate weights.  With this layer's contiguous
    expert sharding ``expert_groups=p`` makes a group a rank, so a token's rows then reach at most
    ``topk_groups`` ranks.  ``balance_bias`` holds a replicated float32 buffer ``expert_bias`` [E]
    (in ``state_dict``, not a Parameter) that is added to the scores for the selection only, keeps
    the last forward's ``counts`` in ``last_counts`` (``last_ids`` and ``last_group_ids`` are the
    last forward's choices), and :meth:`update_balance_bias` moves the bias
    against the load.  The auxiliary loss keeps its formula with ``prob_sum = sum_t s``.  With none
    of these given the layer is what it was, with both routers.

    ``combine_backward="fused"`` takes the combine's two gradients from one pass over the output
    gradient (:func:`combine_tokens` with ``backward="fused"``, the K11 kernel on the GPU) instead of
    a second dispatch and a ``[T, K, d_model]`` product in torch.  The default ``"torch"`` is the
    layer as it was.

    ``drop_policy`` says which assignments a ``capacity_factor`` or a ``source_capacity`` drops:
    ``"position"`` (the default, the layer as it was) the last ones in (token, k) order, ``"probs"`` the
    ones with the lowest gate weight (``dispatchTokens(priority=)`` with the detached gate weights: the
    K15 select on the GPU; ties go to the earlier assignment).  ``"probs"`` without either capacity is
    refused.  A dropped assignment's gate weight gets gradient +0 either way."""

    def __init__(self, comm, d_model: int, d_hidden: int, num_experts: int, top_k: int, seed: int = 0,
                 device=None, dtype=torch.float32, operand=None, capacity_factor=None, source_capacity=None,
                 router: str = "torch", renormalize: bool = False, aux_loss_coef: float = 0.0,
                 z_loss_coef: float = 0.0, combine_backward: str = "torch", score: str = "softmax",
                 expert_groups: Optional[int] = None, topk_groups: Optional[int] = None, routed_scale: float = 1.0,
                 balance_bias: bool = False, drop_policy: str = "position"):
        super().__init__()
        if drop_policy not in DROP_POLICIES:
            raise ValueError(f"drop_policy {drop_policy!r} is not 'position' or 'probs'")
        if drop_policy == "probs" and capacity_factor is None and source_capacity is None:
            raise ValueError("drop_policy='probs' needs capacity_factor or source_capacity: nothing is dropped without one")
        self.drop_policy = drop_policy
        if combine_backward not in COMBINE_BACKWARDS:
            raise ValueError(f"combine_backward {combine_backward!r} is not 'torch' or 'fused'")
        self.combine_backward = combine_backward
        if router not in ("torch", "fused"):
            raise ValueError(f"router {router!r} is not 'torch' or 'fused'")
        if router == "torch" and (renormalize or aux_loss_coef or z_loss_coef):
            raise ValueError("renormalize, aux_loss_coef and z_loss_coef need router='fused'")
        self.router_kind, self.renormalize = router, bool(renormalize)
        self.aux_loss_coef, self.z_loss_coef, self.last_aux_loss = float(aux_loss_coef), float(z_loss_coef), None
        # the group-limited gate (K13): only when one of its arguments is given
        self.grouped = (score != "softmax" or expert_groups is not None or topk_groups is not None
                        or routed_scale != 1.0 or bool(balance_bias))
        if self.grouped:                           # what route_topk_grouped would refuse at the first forward
            from ..ops.device_ops import gate_group_args
            gate_group_args("", num_experts, top_k, score, 1 if expert_groups is None else expert_groups, topk_groups,
                            routed_scale, names=("expert_groups", "topk_groups", "routed_scale", "num_experts"))
        if self.grouped and router != "fused":
            raise ValueError("score, expert_groups, topk_groups, routed_scale and balance_bias need router='fused'")
        if score == "sigmoid" and z_loss_coef:
            raise ValueError("z_loss_coef needs the softmax score: the sigmoid score has no log-sum-exp")
        if topk_groups is not None and expert_groups is None:
            raise ValueError("topk_groups needs expert_groups")
        self.score, self.routed_scale, self.balance_bias = score, float(routed_scale), bool(balance_bias)
        self.expert_groups = 1 if expert_groups is None else expert_groups
        self.topk_groups = self.expert_groups if topk_groups is None else topk_groups
        self.last_counts = self.last_ids = self.last_group_ids = None
        p, r = comm.getSlaveNum(), comm.getRank()
        if num_experts % p:
            raise ValueError(f"num_experts {num_experts} is not a multiple of the {p} ranks")
        if not 1 <= top_k <= num_experts:
            raise ValueError("top_k must be in [1, num_experts]")
        self.comm, self.num_experts, self.top_k, self.operand = comm, num_experts, top_k, operand
        if source_capacity is not None and capacity_factor is not None:
            raise ValueError("give source_capacity or capacity_factor, not both")
        self.capacity_factor, self.source_capacity, self.last_plan = capacity_factor, source_capacity, None
        self.local_experts = num_experts // p
        self.first_expert = r * self.local_experts
        full = self.init_weights(d_model, d_hidden, num_experts, seed)
        lo, hi = self.first_expert, self.first_expert + self.local_experts

        def par(t):
            return torch.nn.Parameter(t.to(device=device, dtype=dtype).contiguous())
        self.router = par(full["router"])
        if self.balance_bias:                      # replicated, moved by update_balance_bias alone
            self.register_buffer("expert_bias", torch.zeros(num_experts, dtype=torch.float32, device=device))
        self.w1, self.b1 = par(full["w1"][lo:hi]), par(full["b1"][lo:hi])
        self.w2, self.b2 = par(full["w2"][lo:hi]), par(full["b2"][lo:hi])

    @staticmethod
    def init_weights(d_model: int, d_hidden: int, num_experts: int, seed: int = 0) -> Dict[str, torch.Tensor]:
        """The whole model's weights (float32, CPU): router [d_model, E], w1 [E, d_model, d_hidden],
        b1 [E, d_hidden], w2 [E, d_hidden, d_model], b2 [E, d_model]."""
        g = torch.Generator().manual_seed(seed)

        def rnd(*shape, fan_in):
            return (torch.rand(*shape, generator=g) * 2 - 1) / fan_in ** 0.5
        return {"router": rnd(d_model, num_experts, fan_in=d_model),
                "w1": rnd(num_experts, d_model, d_hidden, fan_in=d_model),
                "b1": rnd(num_experts, d_hidden, fan_in=d_model),
                "w2": rnd(num_experts, d_hidden, d_model, fan_in=d_hidden),
                "b2": rnd(num_experts, d_model, fan_in=d_hidden)}

    def route(self, x: torch.Tensor):
        """(gate weights float32 [T, K], expert ids int64 [T, K]): softmax over the router's logits,
        top-k, the k-th largest first."""
        probs = torch.softmax((x @ self.router).to(torch.float32), dim=-1)
        return torch.topk(probs, self.top_k, dim=-1)

    def route_fused(self, x: torch.Tensor):
        """:meth:`route` through :func:`route_topk`; stores ``last_aux_loss``."""
        T, E, K = x.shape[0], self.num_experts, self.top_k
        if self.grouped:
            res = route_topk_grouped(x @ self.router, K, score=self.score,
                                     bias=self.expert_bias if self.balance_bias else None, n_group=self.expert_groups,
                                     topk_group=self.topk_groups, renormalize=self.renormalize, scale=self.routed_scale,
                                     stats=self.aux_loss_coef != 0.0 or self.balance_bias)
            self.last_ids, self.last_group_ids = res.ids, res.group_ids
            if self.balance_bias:
                self.last_counts = res.counts
        else:
            res = route_topk(x @ self.router, K, self.renormalize, stats=self.aux_loss_coef != 0.0)
        aux = res.weights.new_zeros(())
        if T and self.aux_loss_coef != 0.0:
            aux = aux + self.aux_loss_coef * E * ((res.counts.to(torch.float32) / (T * K)) * (res.prob_sum / T)).sum()
        if T and self.z_loss_coef != 0.0:
            aux = aux + self.z_loss_coef * (res.lse * res.lse).mean()
        self.last_aux_loss = aux
        return res.weights, res.ids

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        w, ids = self.route_fused(x) if self.router_kind == "fused" else self.route(x)
        rows, plan = dispatch_tokens(self.comm, x, ids, self.num_experts, self.operand,
                                     capacity_factor=self.capacity_factor, source_capacity=self.source_capacity,
                                     priority=w.detach().contiguous() if self.drop_policy == "probs" else None)
        self.last_plan = plan
        if self.source_capacity is not None:
            # [el, p*S, d]: one pair of batched GEMMs whatever the ids were (a pad row's output is the
            # biases' and is never read back; its gradient row is zero)
            h = torch.relu(torch.baddbmm(self.b1.unsqueeze(1), rows, self.w1))
            y = torch.baddbmm(self.b2.unsqueeze(1), h, self.w2)
            return combine_tokens(self.comm, y, plan, w.contiguous(), self.operand, self.combine_backward)
        outs, off = [], 0
        for e, c in enumerate(plan.expert_counts):
            h = torch.relu(rows[off:off + c] @ self.w1[e] + self.b1[e])
            outs.append(h @ self.w2[e] + self.b2[e])
            off += c
        y = torch.cat(outs) if outs else rows
        return combine_tokens(self.comm, y, plan, w.contiguous(), self.operand, self.combine_backward)

    def update_balance_bias(self, rate: float) -> None:
        """Auxiliary-loss-free load balancing, a collective, called after the optimizer step: the
        last forward's ``counts`` are summed over the ranks (the communicator's int64 sum allreduce)
        and ``expert_bias += rate * sign(mean(load) - load)``, so an expert under the mean load is
        chosen more often from the next step on.  Every rank ends with the same bias bits."""
        if not self.balance_bias:
            raise ValueError("update_balance_bias needs balance_bias=True")
        if self.last_counts is None:
            raise ValueError("update_balance_bias needs a forward pass first")
        load = self.last_counts.to(torch.int64).contiguous().clone()
        if self.comm.getSlaveNum() > 1:
            self.comm.allreduceArray(load, Operands.LONG_OPERAND(), Operators.Long.SUM, 0, load.numel())
        with torch.no_grad():
            load = load.to(torch.float32)
            self.expert_bias.add_(torch.sign(load.mean() - load), alpha=float(rate))

    def sync_gradients(self) -> None:
        p = self.comm.getSlaveNum()
        if p == 1:
            return
        for q in (self.w1, self.b1, self.w2, self.b2):
            if q.grad is not None:
                q.grad.mul_(1.0 / p)
        g = self.router.grad if self.router.grad is not None else torch.zeros_like(self.router)
        flat = g.contiguous().view(-1)
        operand = {torch.float32: Operands.FLOAT_OPERAND, torch.bfloat16: Operands.BF16_OPERAND,
                   torch.float16: Operands.HALF_OPERAND}[flat.dtype]()
        self.comm.allreduceArray(flat, operand, Operators.Float.SUM, 0, flat.numel(), scale=1.0 / p)
        self.router.grad = flat.view_as(self.router)
