"""What the group-limited router-gate tests share (tests/test_moe_gate_group_*.py): the definition of
the gate in float64 torch on the CPU with torch autograd, the derived error bounds (DESIGN "K13"),
the tolerance-aware selection check, the separated fixtures and their separation condition, and a
single-process model that holds every expert and computes the same router in plain torch, next to the
rank function that trains ``ExpertParallelMoE`` with the grouped gate beside it."""
import functools

import torch

import moe_gate_ref
import moe_model_ref
from moe_gate_ref import GRAD_SETS, U, gradients, inside, pick, uniform_logits  # noqa: F401
from moe_model_ref import D_HIDDEN, D_MODEL, LR, SEED, STEPS

NEG = float("-inf")
SEPARATION = 2.0 ** -10


# ---------------------------------------------------------------- the definition, float64
def scores64(l64, score):
    if score == "softmax":
        m = l64.max(dim=-1, keepdim=True).values.detach()
        lse = (m + torch.log(torch.exp(l64 - m).sum(dim=-1, keepdim=True))).squeeze(-1)
        return torch.exp(l64 - lse.unsqueeze(1)), lse
    # a masked column (-inf): score 0 and gradient 0, where autograd of exp(inf) would give inf * 0
    safe = torch.where(l64 == NEG, torch.zeros_like(l64), l64)
    return torch.where(l64 == NEG, torch.zeros_like(l64), 1.0 / (1.0 + torch.exp(-safe))), None


def group_scores(c, Gr):
    """[T, Gr]: the sum of a group's two largest selection scores, the largest alone when the second
    is -inf (one live column, or groups of one)."""
    T, E = c.shape
    n = E // Gr
    top = c.view(T, Gr, n).topk(min(2, n), dim=-1).values
    if n == 1:
        return top[..., 0]
    return torch.where(top[..., 1] == NEG, top[..., 0], top[..., 0] + top[..., 1])


def select(key, gs, Gr, Kg, K):
    """(group_ids, ids): the first Kg groups in (score descending, index ascending), then the first K
    columns of those groups in (key descending, column ascending)."""
    T, E = key.shape
    gids = torch.sort(gs, dim=-1, descending=True, stable=True).indices[:, :Kg]
    inside_ = torch.zeros(T, Gr, dtype=torch.bool).scatter_(1, gids, True).repeat_interleave(E // Gr, dim=1)
    order = torch.sort(key, dim=-1, descending=True, stable=True).indices
    keep = torch.sort(inside_.gather(1, order).to(torch.int8), dim=-1, descending=True, stable=True).indices
    return gids, order.gather(1, keep)[:, :K]


class Reference:
    """The float64 definition of one case and the bounds of its float32 evaluations (DESIGN "K13")."""

    def __init__(self, logits, K, score, bias, Gr, Kg, renormalize, scale):
        self.logits, self.K, self.score, self.bias = logits, K, score, bias
        self.Gr, self.Kg, self.renormalize, self.scale = Gr, Kg, renormalize, scale
        self.T, self.E = logits.shape
        self.l64 = logits.to(torch.float64).requires_grad_(True)
        self.s, self.lse = scores64(self.l64, score)
        s = self.s.detach()
        masked = logits.to(torch.float64) == NEG
        c = s if bias is None else s + bias.to(torch.float64)
        self.c = torch.where(masked, torch.full_like(c, NEG), c)
        self.gs = group_scores(self.c, Gr)
        # without a bias the order is the logits' own, exactly
        self.group_ids, self.ids = select(logits.to(torch.float64) if bias is None else self.c, self.gs, Gr, Kg, K)
        # the score's relative error: K10's B for the softmax, 16 u for the sigmoid (|l| <= 32)
        self.B = moe_gate_ref.bound_b(logits) if score == "softmax" else 16 * U
        d = self.B * s + (0 if bias is None else U * self.c.abs())
        self.delta = torch.where(masked, torch.zeros_like(d), d)                       # on c
        dmax = self.delta.view(self.T, Gr, self.E // Gr).max(dim=-1).values
        self.delta_g = torch.where(self.gs == NEG, torch.zeros_like(dmax), 2 * dmax + U * self.gs.abs())
        self.prob_sum = self.s.sum(dim=0)

    def weights(self, ids):
        """(w64, S64) for the ids an evaluation chose, differentiable."""
        q = self.s.gather(1, ids)
        S = q[:, 0]
        for k in range(1, q.shape[1]):
            S = S + q[:, k]
        w = q / S.unsqueeze(1) if self.renormalize else q
        return w * self.scale, S

    def weights_bound(self, ids):
        b = (2 * self.B + (self.K + 1) * U if self.renormalize else self.B) + U         # + one rounding for the scale
        return b * self.weights(ids)[0].detach()

    def lse_bound(self):
        return self.B + U * self.lse.detach().abs()

    def prob_sum_bound(self):
        return (self.B + self.T * U) * self.prob_sum.detach()

    def backward(self, ids, g_w=None, g_lse=None, g_psum=None):
        """(g64, bound): torch autograd of the definition at ``ids`` and |g - g64| <= bound for a
        float32 evaluation rounded once to the logits' dtype."""
        w, S = self.weights(ids)
        loss = self.l64.sum() * 0
        if g_w is not None:
            loss = loss + (w * g_w.to(torch.float64)).sum()
        if g_lse is not None:
            loss = loss + (self.lse * g_lse.to(torch.float64)).sum()
        if g_psum is not None:
            loss = loss + (self.prob_sum * g_psum.to(torch.float64)).sum()
        (g64,) = torch.autograd.grad(loss, self.l64, retain_graph=True)
        s = self.s.detach()
        A = torch.zeros_like(s)
        if g_psum is not None:
            A = A + g_psum.to(torch.float64).abs().unsqueeze(0)
        if g_w is not None:
            gq = g_w.to(torch.float64).abs() * self.scale
            if self.renormalize:
                wn = (w / self.scale).detach()
                gq = (gq + (gq * wn).sum(dim=-1, keepdim=True)) / S.detach().unsqueeze(1)
            A = A.scatter_add(1, ids, gq)
        if self.score == "softmax":
            gl = torch.zeros(self.T, dtype=torch.float64) if g_lse is None else g_lse.to(torch.float64).abs()
            bound = 4 * (self.B + (self.K + 1) * U) * s * (A + (A * s).sum(dim=-1, keepdim=True) + gl.unsqueeze(1))
        else:
            d = s * (1.0 / (1.0 + torch.exp(self.l64.detach())))
            bound = (5 * self.B + (3 * self.K + 7) * U) * d * A
        if self.logits.dtype == torch.bfloat16:
            bound = bound + 2.0 ** -8 * g64.abs()
        elif self.logits.dtype == torch.float16:
            bound = bound + 2.0 ** -11 * g64.abs() + 2.0 ** -25
        return g64, bound

    # ------------------------------------------------------------ the tolerance-aware selection check
    def selection_ok(self, group_ids, ids):
        """None, or what is wrong with (group_ids, ids) as the choice of an evaluation whose
        selection scores lie within ``delta`` and whose group scores within ``delta_g`` of the
        float64 definition."""
        T, E, Gr, Kg, K, n = self.T, self.E, self.Gr, self.Kg, self.K, self.E // self.Gr
        gids, ids = group_ids.to(torch.int64).cpu(), ids.to(torch.int64).cpu()
        if tuple(gids.shape) != (T, Kg) or tuple(ids.shape) != (T, K):
            return "shapes"
        if T == 0:
            return None
        if not bool(((gids >= 0) & (gids < Gr)).all()) or int(torch.sort(gids, dim=-1).values.diff(dim=-1).eq(0).sum()):
            return "groups out of range or repeated"
        chosen = torch.zeros(T, Gr, dtype=torch.bool).scatter_(1, gids, True)
        lo = torch.where(chosen, self.gs + self.delta_g, torch.full_like(self.gs, float("inf"))).min(dim=-1).values
        hi = torch.where(chosen, torch.full_like(self.gs, NEG), self.gs - self.delta_g).max(dim=-1).values
        if not bool((lo >= hi).all()):
            return "an unchosen group scores more than a chosen one by more than the bounds"
        if not bool(((ids >= 0) & (ids < E)).all()) or int(torch.sort(ids, dim=-1).values.diff(dim=-1).eq(0).sum()):
            return "ids out of range or repeated"
        if not bool(chosen.gather(1, ids // n).all()):
            return "an id outside the chosen groups"
        taken = torch.zeros(T, E, dtype=torch.bool).scatter_(1, ids, True)
        eligible = chosen.repeat_interleave(n, dim=1) & ~taken
        lo = torch.where(taken, self.c + self.delta, torch.full_like(self.c, float("inf"))).min(dim=-1).values
        hi = torch.where(eligible, self.c - self.delta, torch.full_like(self.c, NEG)).max(dim=-1).values
        if not bool((lo >= hi).all()):
            return "an unchosen column scores more than a chosen one by more than the bounds"
        ck, dk = self.c.gather(1, ids), self.delta.gather(1, ids)
        if K > 1 and not bool((ck[:, :-1] + dk[:, :-1] >= ck[:, 1:] - dk[:, 1:]).all()):
            return "the chosen columns do not descend"
        return None


def separated(ref):
    """None, or why the fixture is not separated: any two columns of a row and any two groups of a
    row either come from identical inputs (the same logit and bias bits; for groups the same pair
    of them) or differ in float64 by at least 2^-10 relative."""
    T, E, Gr, n = ref.T, ref.E, ref.Gr, ref.E // ref.Gr
    lg = ref.logits.to(torch.float64)
    lg = torch.where(lg == 0, torch.zeros_like(lg), lg)                   # -0 == +0
    b = torch.zeros(E, dtype=torch.float64) if ref.bias is None else ref.bias.to(torch.float64)
    c = ref.c
    same = (lg.unsqueeze(2) == lg.unsqueeze(1)) & (b.view(1, E, 1) == b.view(1, 1, E))
    same = same | ((c.unsqueeze(2) == NEG) & (c.unsqueeze(1) == NEG))
    gap = (c.unsqueeze(2) - c.unsqueeze(1)).abs()
    big = torch.maximum(c.unsqueeze(2).abs(), c.unsqueeze(1).abs())
    ok = same | (gap >= SEPARATION * big) | torch.isinf(gap)
    if not bool(ok.all()):
        return "two columns too close"
    # a group's pair: its two largest (c, logit, bias) by c
    top = c.view(T, Gr, n).topk(min(2, n), dim=-1)
    col = top.indices + (torch.arange(Gr) * n).view(1, Gr, 1)
    pl = lg.gather(1, col.view(T, -1)).view(T, Gr, -1)
    pb = b[col.view(-1)].view(T, Gr, -1)
    pair = torch.cat([torch.where(top.values == NEG, torch.full_like(pl, NEG), pl),
                      torch.where(top.values == NEG, torch.zeros_like(pb), pb)], dim=-1)
    same = (pair.unsqueeze(2) == pair.unsqueeze(1)).all(dim=-1)
    gs = ref.gs
    gap = (gs.unsqueeze(2) - gs.unsqueeze(1)).abs()
    big = torch.maximum(gs.unsqueeze(2).abs(), gs.unsqueeze(1).abs())
    ok = same | (gap >= SEPARATION * big) | torch.isinf(gap) | ((gs.unsqueeze(2) == NEG) & (gs.unsqueeze(1) == NEG))
    if not bool(ok.all()):
        return "two groups too close"
    return None


# ---------------------------------------------------------------- inputs
def level_logits(T, E, Gr, seed, dtype=torch.float32, levels=(0, 1, 2, 3, 4), masks=True):
    """Many ties, separated: small non-negative integer logits (exact in every dtype; symmetric
    integers would make sigma(2) + sigma(-2) tie with sigma(0) + sigma(0) in exact arithmetic only),
    every group capped at a level of its own so that the group scores vary; row 0 all equal; -inf
    masks, among them a group masked whole and (row 1) a row with one live column."""
    g = torch.Generator().manual_seed(seed)
    lv = torch.tensor(levels, dtype=torch.float32)
    cap = torch.randint(1, len(levels) + 1, (T, Gr), generator=g).repeat_interleave(E // Gr, dim=1)
    lg = lv[(torch.rand(T, E, generator=g) * cap).long().clamp(max=len(levels) - 1)]
    if masks:
        lg = torch.where(torch.rand(T, E, generator=g) < 0.2, torch.full_like(lg, NEG), lg)
        if T > 3:
            lg[3, :E // Gr] = NEG                        # group 0 has no live column
        lg[~torch.isfinite(lg).any(dim=-1), 0] = 1.0
        if T > 1:
            lg[1] = NEG
            lg[1, E // 2] = 2.0
    if T:
        lg[0] = 1.0
    return lg.to(dtype)


def level_bias(E, Gr, seed, per_group):
    """A separated bias: two levels {0, 0.3} per column (for Gr = 1), or one level 0.25 * pi(g) per
    group (with groups)."""
    g = torch.Generator().manual_seed(seed)
    if per_group:
        return (0.25 * torch.randperm(Gr, generator=g).to(torch.float32)).repeat_interleave(E // Gr)
    return 0.3 * (torch.rand(E, generator=g) < 0.5).to(torch.float32)


def random_bias(E, seed):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(E, generator=g) - 0.5) * 0.2).to(torch.float32)


# (name, E, Gr, Kg, K, score, bias kind): the separated fixtures, whose ids are exact
SEPARATED = [
    ("groups", 8, 4, 2, 2, "sigmoid", None), ("groups", 6, 3, 2, 4, "sigmoid", None),
    ("groups", 60, 5, 3, 6, "softmax", None), ("groups", 64, 8, 4, 8, "sigmoid", None),
    ("groups", 256, 8, 4, 8, "sigmoid", None), ("groups", 260, 4, 1, 16, "softmax", None),
    ("groups", 2048, 32, 8, 16, "sigmoid", None),
    ("bias", 64, 1, 1, 8, "sigmoid", "column"), ("bias", 260, 1, 1, 16, "softmax", "column"),
    ("both", 64, 8, 4, 8, "sigmoid", "group"), ("both", 256, 8, 4, 8, "sigmoid", "group"),
]


@functools.lru_cache(maxsize=None)
def separated_case(i, T, dtype, renormalize=True, scale=2.5):
    """(logits, bias, Reference) of SEPARATED[i]; one reference per case, left unchanged."""
    kind, E, Gr, Kg, K, score, bk = SEPARATED[i]
    levels = (0, 2, 4) if kind == "both" else (0, 1, 2, 3, 4)
    logits = level_logits(T, E, Gr, 600 + i, getattr(torch, dtype), levels)
    bias = None if bk is None else level_bias(E, Gr, 700 + i, bk == "group")
    return logits, bias, Reference(logits, K, score, bias, Gr, Kg, renormalize, scale)


@functools.lru_cache(maxsize=None)
def uniform_case(T, E, Gr, Kg, K, score, with_bias, renormalize, scale, R, seed, dtype):
    logits = uniform_logits(T, E, R, seed, getattr(torch, dtype))
    bias = random_bias(E, seed + 1) if with_bias else None
    return logits, bias, Reference(logits, K, score, bias, Gr, Kg, renormalize, scale)


# ---------------------------------------------------------------- the model
EXPERTS, GROUPS, TOPK_GROUPS, TOP_K, SCALE, AUX, RATE = 8, 4, 2, 2, 2.5, 0.01, 0.01


class DenseGroupedMoE(torch.nn.Module):
    """Every expert in one process; the router as a user writes it in plain torch: sigmoid, the
    groups' top-2 sums, top-k groups, a mask, top-k experts, gather, renormalise, scale."""

    def __init__(self, full):
        super().__init__()
        for name, t in full.items():
            setattr(self, name, torch.nn.Parameter(t.clone()))
        self.register_buffer("expert_bias", torch.zeros(EXPERTS))

    def gate(self, x):
        logits = (x @ self.router).to(torch.float32)
        T = logits.shape[0]
        s = 1.0 / (1.0 + torch.exp(-logits))
        c = (s + self.expert_bias).detach()
        gs = c.view(T, GROUPS, -1).topk(2, dim=-1).values.sum(dim=-1)
        gids = gs.topk(TOPK_GROUPS, dim=-1).indices
        mask = torch.zeros_like(gs).scatter_(1, gids, 1.0).repeat_interleave(EXPERTS // GROUPS, dim=1)
        ids = c.masked_fill(mask == 0, NEG).topk(TOP_K, dim=-1).indices
        w = s.gather(1, ids)
        return s, ids, w / w.sum(dim=-1, keepdim=True) * SCALE, gids

    def aux(self, x):
        s, ids, _, _ = self.gate(x)
        T = s.shape[0]
        counts = torch.bincount(ids.reshape(-1), minlength=EXPERTS).to(torch.float32)
        return AUX * EXPERTS * ((counts / (T * TOP_K)) * (s.sum(dim=0) / T)).sum()

    def forward(self, x):
        _, ids, w, _ = self.gate(x)
        out = torch.zeros_like(x)
        for k in range(TOP_K):
            for e in range(EXPERTS):
                m = ids[:, k] == e
                if bool(m.any()):
                    y = torch.relu(x[m] @ self.w1[e] + self.b1[e]) @ self.w2[e] + self.b2[e]
                    out = out.index_put((m.nonzero().view(-1),), w[m, k].unsqueeze(1) * y, accumulate=True)
        return out


def train(comm, device):
    """Per-step (this rank's loss, the single-process model's loss over every rank's tokens), the
    expert drift, and per step: the bias bits of this rank, whether the bias equals the reference's
    update from the summed counts, whether the two models chose the same experts, and whether every
    token's ids stayed inside its ``TOPK_GROUPS`` groups."""
    from mp4x.models.moe import ExpertParallelMoE
    r, p = comm.getRank(), comm.getSlaveNum()
    model = ExpertParallelMoE(comm, D_MODEL, D_HIDDEN, EXPERTS, TOP_K, seed=SEED, device=device, router="fused",
                              score="sigmoid", expert_groups=GROUPS, topk_groups=TOPK_GROUPS, renormalize=True,
                              routed_scale=SCALE, balance_bias=True, aux_loss_coef=AUX)
    ref = DenseGroupedMoE(ExpertParallelMoE.init_weights(D_MODEL, D_HIDDEN, EXPERTS, SEED)).to(device)
    data = [tuple(t.to(device) for t in moe_model_ref.batch(i)) for i in range(p)]
    allx, ally = torch.cat([d[0] for d in data]), torch.cat([d[1] for d in data])
    opt = torch.optim.SGD(model.parameters(), lr=LR)
    ropt = torch.optim.SGD(ref.parameters(), lr=LR)
    mine, whole, steps = [], [], []
    n = EXPERTS // GROUPS
    for _ in range(STEPS):
        with torch.no_grad():
            _, rids, _, _ = ref.gate(allx)
        loss = ((model(data[r][0]) - data[r][1]) ** 2).mean() + model.last_aux_loss
        ids, gids = model.last_ids, model.last_group_ids.to(torch.int64)
        same_ids = torch.equal(ids.cpu(), rids[r * ids.shape[0]:(r + 1) * ids.shape[0]].cpu())
        groups_of = ids // n
        in_groups = bool((groups_of.unsqueeze(2) == gids.unsqueeze(1)).any(dim=-1).all())
        fan_out = max(len(set(row)) for row in groups_of.tolist())
        opt.zero_grad()
        loss.backward()
        model.sync_gradients()
        opt.step()
        model.update_balance_bias(RATE)
        rloss = ((ref(allx) - ally) ** 2).mean() + sum(ref.aux(d[0]) for d in data) / p
        ropt.zero_grad()
        rloss.backward()
        ropt.step()
        with torch.no_grad():
            load = torch.bincount(rids.reshape(-1), minlength=EXPERTS).to(torch.float32)
            ref.expert_bias.add_(torch.sign(load.mean() - load), alpha=RATE)
        mine.append(float(loss))
        whole.append(float(rloss))
        steps.append(dict(bias=model.expert_bias.cpu().view(torch.int32).tolist(),
                          bias_ok=torch.equal(model.expert_bias.cpu(), ref.expert_bias.cpu()), same_ids=same_ids,
                          in_groups=in_groups and fan_out <= TOPK_GROUPS))
    lo = model.first_expert
    drift = float((model.w2.detach() - ref.w2.detach()[lo:lo + model.local_experts]).abs().max())
    in_state = "expert_bias" in model.state_dict() and "expert_bias" not in dict(model.named_parameters())
    return mine, whole, drift, steps, in_state


def default_untouched(comm, device, router):
    """Without the new arguments the layer calls none of the new code and gives, bit for bit, the
    output of the steps it took before, re-evaluated here: for ``router`` "torch" and "fused"."""
    from mp4x.models import moe
    from moe_model_ref import EXPERTS as E4, TOP_K as K2
    r = comm.getRank()
    kw = dict(router="fused", renormalize=True, aux_loss_coef=AUX) if router == "fused" else {}
    model = moe.ExpertParallelMoE(comm, D_MODEL, D_HIDDEN, E4, K2, seed=SEED, device=device, **kw)
    x = moe_model_ref.batch(r)[0].to(device)
    calls, real = [], moe.route_topk_grouped
    moe.route_topk_grouped = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        out = model(x)
    finally:
        moe.route_topk_grouped = real
    if router == "fused":
        res = moe.route_topk(x @ model.router, K2, True, stats=True)
        w, ids = res.weights, res.ids
        aux = AUX * E4 * ((res.counts.to(torch.float32) / (x.shape[0] * K2)) * (res.prob_sum / x.shape[0])).sum()
        aux_ok = moe_model_ref.same_bits(model.last_aux_loss.detach().view(1), (res.lse.new_zeros(()) + aux).detach().view(1))
    else:
        w, ids = torch.topk(torch.softmax((x @ model.router).to(torch.float32), dim=-1), K2, dim=-1)
        aux_ok = model.last_aux_loss is None
    rows, plan = moe.dispatch_tokens(comm, x, ids, E4)
    outs, off = [], 0
    for e, c in enumerate(plan.expert_counts):
        h = torch.relu(rows[off:off + c] @ model.w1[e] + model.b1[e])
        outs.append(h @ model.w2[e] + model.b2[e])
        off += c
    want = moe.combine_tokens(comm, torch.cat(outs) if outs else rows, plan, w.contiguous())
    return dict(calls=len(calls), out=moe_model_ref.same_bits(out.detach(), want.detach()), aux=aux_ok,
                grouped=model.grouped, buffers=[n for n, _ in model.named_buffers()])
