"""What the router-gate tests share (tests/test_moe_gate_*.py): the definition of the gate in float64
torch on the CPU with torch autograd, the derived error bounds (DESIGN "K10"), the input cases, and
a single-process model that holds every expert and computes the same router and the same two
auxiliary losses per rank in plain torch, next to the rank function that trains
``ExpertParallelMoE(router="fused")`` beside it."""
import functools

import torch

import moe_model_ref
from moe_model_ref import D_HIDDEN, D_MODEL, EXPERTS, LR, SEED, STEPS, TOP_K

U = 2.0 ** -24
AUX, ZL = 0.01, 0.001


# ---------------------------------------------------------------- the definition, float64
def order_ids(logits, K):
    """The first K columns in (logit descending, index ascending): a stable descending sort."""
    return torch.sort(logits.to(torch.float64), dim=-1, descending=True, stable=True).indices[:, :K]


def definition(l64, ids, renormalize):
    """(weights, lse, prob_sum, p, s) of float64 logits, differentiable."""
    m = l64.max(dim=-1, keepdim=True).values.detach()
    lse = (m + torch.log(torch.exp(l64 - m).sum(dim=-1, keepdim=True))).squeeze(-1)
    p = torch.exp(l64 - lse.unsqueeze(1))
    w = p.gather(1, ids)
    s = w[:, 0]
    for k in range(1, w.shape[1]):
        s = s + w[:, k]
    if renormalize:
        w = w / s.unsqueeze(1)
    return w, lse, p.sum(dim=0), p, s


def spread(logits):
    """R: the largest (max - min finite logit) of any row."""
    lg = logits.to(torch.float64)
    fin = torch.isfinite(lg)
    hi = torch.where(fin, lg, torch.full_like(lg, -1e300)).max(dim=-1).values
    lo = torch.where(fin, lg, torch.full_like(lg, 1e300)).min(dim=-1).values
    return float((hi - lo).clamp(min=0).max()) if lg.shape[0] else 0.0


def bound_b(logits):
    return (2 * spread(logits) + logits.shape[1] / 16 + 16) * U


class Reference:
    """The float64 forward of (logits, K, renormalize) and the bounds of its float32 evaluations."""

    def __init__(self, logits, K, renormalize):
        self.logits, self.K, self.renormalize = logits, K, renormalize
        self.T, self.E = logits.shape
        self.ids = order_ids(logits, K)
        self.l64 = logits.to(torch.float64).requires_grad_(True)
        self.w, self.lse, self.prob_sum, self.p, self.s = definition(self.l64, self.ids, renormalize)
        self.counts = torch.bincount(self.ids.reshape(-1), minlength=self.E)
        self.B = bound_b(logits)

    # forward bounds: |x - x64| <= bound, elementwise
    def weights_bound(self):
        b = 2 * self.B + (self.K + 1) * U if self.renormalize else self.B
        return b * self.w.detach()

    def lse_bound(self):
        return self.B + U * self.lse.detach().abs()

    def prob_sum_bound(self):
        return (self.B + self.T * U) * self.prob_sum.detach()

    def backward(self, g_w=None, g_lse=None, g_psum=None):
        """(g64, bound): torch autograd of the definition and |g - g64| <= bound for a float32
        evaluation rounded once to the logits' dtype."""
        loss = self.l64.sum() * 0
        if g_w is not None:
            loss = loss + (self.w * g_w.to(torch.float64)).sum()
        if g_lse is not None:
            loss = loss + (self.lse * g_lse.to(torch.float64)).sum()
        if g_psum is not None:
            loss = loss + (self.prob_sum * g_psum.to(torch.float64)).sum()
        (g64,) = torch.autograd.grad(loss, self.l64, retain_graph=True)
        p = self.p.detach()
        A = torch.zeros_like(p)
        if g_psum is not None:
            A = A + g_psum.to(torch.float64).abs().unsqueeze(0)
        if g_w is not None:
            gq = g_w.to(torch.float64).abs()
            if self.renormalize:
                gq = (gq + (gq * self.w.detach()).sum(dim=-1, keepdim=True)) / self.s.detach().unsqueeze(1)
            A = A.scatter_add(1, self.ids, gq)
        gl = torch.zeros(self.T, dtype=torch.float64) if g_lse is None else g_lse.to(torch.float64).abs()
        bound = 4 * (self.B + self.K * U) * p * (A + (A * p).sum(dim=-1, keepdim=True) + gl.unsqueeze(1))
        # one rounding to a 16-bit dtype: the unit roundoff of the format (8 / 11 significant bits:
        # half an ulp is 2^-8 / 2^-11 of a value at the bottom of its binade) in the normal range;
        # half a subnormal step of float16 (2^-25) below it, where a relative bound cannot hold
        if self.logits.dtype == torch.bfloat16:
            bound = bound + 2.0 ** -8 * g64.abs()
        elif self.logits.dtype == torch.float16:
            bound = bound + 2.0 ** -11 * g64.abs() + 2.0 ** -25
        return g64, bound


def inside(got, want, bound):
    """(ok, worst ratio) of |got - want| <= bound elementwise (an exact match passes a zero bound)."""
    err = (got.detach().to(torch.float64).cpu() - want.detach()).abs()
    if err.numel() == 0:
        return True, 0.0
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp(min=1e-300))
    return bool((err <= bound).all()), float(ratio.max())


# ---------------------------------------------------------------- inputs
def uniform_logits(T, E, R, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(T, E, generator=g) - 0.5) * R).to(dtype)


def tie_logits(T, E, seed, dtype=torch.float32):
    """Many ties: integer-valued logits in [-2, 2] (exact in every dtype), row 0 all equal, signed
    zeros, and -inf masks (row 1 masked except one column, when there is a row 1)."""
    g = torch.Generator().manual_seed(seed)
    lg = torch.randint(-2, 3, (T, E), generator=g).to(torch.float32)
    lg = torch.where((lg == 0) & (torch.rand(T, E, generator=g) < 0.5), torch.full_like(lg, -0.0), lg)
    lg = torch.where(torch.rand(T, E, generator=g) < 0.25, torch.full_like(lg, float("-inf")), lg)
    lg[~torch.isfinite(lg).any(dim=-1), 0] = 1.0           # no row is masked whole
    if T:
        lg[0] = 1.0
    if T > 1:
        lg[1] = float("-inf")
        lg[1, E // 2] = 0.5
    if T > 2:
        lg[2, 0] = 3.0                                  # a finite maximum in every later check of row 2
    return lg.to(dtype)


def gradients(T, E, K, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(T, K, generator=g), torch.randn(T, generator=g), torch.randn(E, generator=g))


GRAD_SETS = [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]


def pick(grads, which):
    return tuple(g if on else None for g, on in zip(grads, which))


# ---------------------------------------------------------------- the model
class DenseGateMoE(torch.nn.Module):
    """Every expert in one process, the router by the definition: ids from the stable sort of the
    logits, gates = softmax probabilities renormalised over the chosen K; ``aux(x)`` is the rank's
    auxiliary loss of its tokens x."""

    def __init__(self, full, top_k):
        super().__init__()
        self.top_k = top_k
        for name, t in full.items():
            setattr(self, name, torch.nn.Parameter(t.clone()))

    def gate(self, x):
        logits = (x @ self.router).to(torch.float32)
        p = torch.softmax(logits, dim=-1)
        ids = torch.sort(logits.detach(), dim=-1, descending=True, stable=True).indices[:, :self.top_k]
        w = p.gather(1, ids)
        return logits, p, ids, w / w.sum(dim=-1, keepdim=True)

    def aux(self, x):
        logits, p, ids, _ = self.gate(x)
        T, E = logits.shape
        counts = torch.bincount(ids.reshape(-1), minlength=E).to(torch.float32)
        lse = torch.logsumexp(logits, dim=-1)
        return AUX * E * ((counts / (T * self.top_k)) * (p.sum(dim=0) / T)).sum() + ZL * (lse ** 2).mean()

    def forward(self, x):
        _, _, ids, w = self.gate(x)
        out = torch.zeros_like(x)
        for k in range(self.top_k):
            for e in range(self.w1.shape[0]):
                m = ids[:, k] == e
                if bool(m.any()):
                    y = torch.relu(x[m] @ self.w1[e] + self.b1[e]) @ self.w2[e] + self.b2[e]
                    out = out.index_put((m.nonzero().view(-1),), w[m, k].unsqueeze(1) * y, accumulate=True)
        return out


def train(comm, device):
    """Per-step (this rank's loss, the single-process model's loss over every rank's tokens), the
    expert drift, and whether the auxiliary losses alone reach the router's gradient."""
    from mp4x.models.moe import ExpertParallelMoE
    r, p = comm.getRank(), comm.getSlaveNum()
    model = ExpertParallelMoE(comm, D_MODEL, D_HIDDEN, EXPERTS, TOP_K, seed=SEED, device=device, router="fused",
                              renormalize=True, aux_loss_coef=AUX, z_loss_coef=ZL)
    ref = DenseGateMoE(ExpertParallelMoE.init_weights(D_MODEL, D_HIDDEN, EXPERTS, SEED), TOP_K).to(device)
    data = [tuple(t.to(device) for t in moe_model_ref.batch(i)) for i in range(p)]
    allx, ally = torch.cat([d[0] for d in data]), torch.cat([d[1] for d in data])

    # the auxiliary losses alone: g_psum and g_lse are the only gradients that reach the gate
    model(data[r][0])
    model.last_aux_loss.backward()
    aux_only = float(model.router.grad.abs().max())
    ref.aux(data[r][0]).backward()
    aux_err = float((model.router.grad - ref.router.grad).abs().max())
    model.zero_grad()
    ref.zero_grad()

    opt = torch.optim.SGD(model.parameters(), lr=LR)
    ropt = torch.optim.SGD(ref.parameters(), lr=LR)
    mine, whole = [], []
    for _ in range(STEPS):
        loss = ((model(data[r][0]) - data[r][1]) ** 2).mean() + model.last_aux_loss
        opt.zero_grad()
        loss.backward()
        model.sync_gradients()
        opt.step()
        rloss = ((ref(allx) - ally) ** 2).mean() + sum(ref.aux(d[0]) for d in data) / p
        ropt.zero_grad()
        rloss.backward()
        ropt.step()
        mine.append(float(loss))
        whole.append(float(rloss))
    lo = model.first_expert
    drift = float((model.w2.detach() - ref.w2.detach()[lo:lo + model.local_experts]).abs().max())
    return mine, whole, drift, aux_only, aux_err


def default_untouched(comm, device):
    """router="torch" (the default) is the layer as it was: its output equals, bit for bit, the
    layer's own steps with ``route()`` re-evaluated here, and route_topk is never entered."""
    from mp4x.models import moe
    r = comm.getRank()
    model = moe.ExpertParallelMoE(comm, D_MODEL, D_HIDDEN, EXPERTS, TOP_K, seed=SEED, device=device)
    x = moe_model_ref.batch(r)[0].to(device)
    calls, real = [], moe.route_topk
    moe.route_topk = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        out = model(x)
    finally:
        moe.route_topk = real
    probs = torch.softmax((x @ model.router).to(torch.float32), dim=-1)
    w, ids = torch.topk(probs, TOP_K, dim=-1)
    rw, rids = model.route(x)
    rows, plan = moe.dispatch_tokens(comm, x, ids, EXPERTS)
    outs, off = [], 0
    for e, c in enumerate(plan.expert_counts):
        h = torch.relu(rows[off:off + c] @ model.w1[e] + model.b1[e])
        outs.append(h @ model.w2[e] + model.b2[e])
        off += c
    want = moe.combine_tokens(comm, torch.cat(outs) if outs else rows, plan, w.contiguous())
    return dict(calls=len(calls), route=torch.equal(rw, w) and torch.equal(rids, ids),
                out=moe_model_ref.same_bits(out.detach(), want.detach()), aux=model.last_aux_loss is None,
                kind=model.router_kind)


@functools.lru_cache(maxsize=None)
def cached_reference(kind, T, E, K, renormalize, R, seed, dtype):
    """One float64 reference per case, shared by the tests that need it and left unchanged."""
    dt = getattr(torch, dtype)
    logits = tie_logits(T, E, seed, dt) if kind == "ties" else uniform_logits(T, E, R, seed, dt)
    return logits, Reference(logits, K, renormalize)
