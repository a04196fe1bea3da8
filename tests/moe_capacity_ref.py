"""The expert capacity of dispatchTokens in plain torch on the CPU, written from the global definition
(not from the quota formula), and the (case, capacity) pairs the capacity tests run.  Shared by
tests/test_moe_capacity_cpu.py, the capacity kernel / API tests on the GPU and the capacity model
tests.

Every rank's flattened assignments are concatenated rank-major and walked in that order with one
counter per expert: an assignment with expert e is kept while e's counter is below the capacity C.
A clipped assignment's id becomes -1; with those ids tests/moe_ref.py gives the whole expected
result unchanged (a capped call IS the uncapped call on the clipped ids).
"""
import torch

import moe_model_ref
import moe_ref
from moe_ref import same_bits  # noqa: F401  (re-exported for the tests)

NO_CLIP = 1 << 20            # above every case's demand

# (case of moe_ref.CASES, C) -> rows every rank keeps, by rank count; asserted by clipped_case(), so a
# case cannot silently stop clipping
KEPT = {
    ("A", 7): {2: [49, 0], 3: [77, 0, 0]},            # an empty rank and an empty expert; p = 3: a rank with tokens sends nothing
    ("A", 40): {2: [280, 0], 3: [431, 0, 9]},         # some experts clipped, others not: later bases shift
    ("B", 3): {2: [6, 0], 3: [7, 1, 1]},              # one local expert (no regroup); cut inside the first wave
    ("C", 6): {2: [300, 84], 3: [300, 276, 0]},       # 64 distinct experts per wave; partial or zero quotas on the last rank
    ("D", 300): {2: [260, 40], 3: [260, 40, 0]},      # one expert, cut inside tile 0 of rank 1; V = 65, tiles split
    ("D", 518): {2: [260, 258], 3: [260, 258, 0]},    # cut in the second tile, two rows in
}
# the unclipped totals of case A, for the record the table was made against
DEMAND_A = {2: [472, 0], 3: [472, 0, 470]}
TABLE = sorted(KEPT)
EVERY = TABLE + [(name, 1) for name in sorted(moe_ref.CASES)] + [(name, NO_CLIP) for name in sorted(moe_ref.CASES)]


def clip_ids(ids_per_rank, E, C):
    """(per rank: the ids with every clipped assignment set to -1; keep[i][e]; per rank: clipped).
    ``C``: the capacity, or one per expert (the kernel tests give quotas directly)."""
    C = [C] * E if isinstance(C, int) else list(C)
    taken = [0] * E
    out, keep, clipped = [], [], []
    for ids in ids_per_rank:                                     # rank-major ...
        flat = ids.reshape(-1).clone()
        kept_here, dropped = [0] * E, 0
        for a in range(flat.numel()):                            # ... then the sender's assignment index
            e = int(flat[a])
            if e < 0 or e >= E:
                continue
            if taken[e] < C[e]:
                taken[e] += 1
                kept_here[e] += 1
            else:
                flat[a] = -1
                dropped += 1
        out.append(flat.view(ids.shape))
        keep.append(kept_here)
        clipped.append(dropped)
    return out, keep, clipped


def clipped_case(name, p, C):
    """Per rank (x, clipped ids, w, E) as moe_ref.case gives them, their routes, and
    dict(ids=the unclipped ids, keep, clipped, demand) of the whole job."""
    per_rank, raw_routes = moe_ref.check_case_properties(name, p)
    E = per_rank[0][3]
    ids, keep, clipped = clip_ids([c[1] for c in per_rank], E, C)
    demand = [rt[0][:E].tolist() for rt in raw_routes]
    if (name, C) in KEPT and p in KEPT[(name, C)]:
        assert [sum(k) for k in keep] == KEPT[(name, C)][p], (name, C, p, [sum(k) for k in keep])
        assert sum(clipped) > 0
    if name == "A" and p in DEMAND_A:
        assert [sum(d) for d in demand] == DEMAND_A[p]
    if C == NO_CLIP:
        assert sum(clipped) == 0
    assert [sum(d) - sum(k) for d, k in zip(demand, keep)] == clipped
    capped = [(x, cid, w, E) for (x, _, w, _), cid in zip(per_rank, ids)]
    routes = [moe_ref.ref_route(cid, E) for cid in ids]
    return capped, routes, dict(ids=[c[1] for c in per_rank], keep=keep, clipped=clipped, demand=demand)


_MEMO = {}


def end_to_end(name, p, C):
    """moe_ref.end_to_end under the capacity C: per rank dict(x, ids (unclipped), clipped_ids, w, E,
    rows, expert_counts, mat, emat, send, slots, back, out, keep, clipped, demand).  Computed once
    per (name, p, C); the tests leave it unchanged."""
    key = (name, p, C)
    if key in _MEMO:
        return _MEMO[key]
    capped, routes, info = clipped_case(name, p, C)
    E = capped[0][3]
    el = E // p
    K = capped[0][1].shape[1]
    sends = [moe_ref.ref_send(x, rt[2], K) for (x, _, _, _), rt in zip(capped, routes)]
    ex = moe_ref.ref_exchange(sends, routes, E)
    outs = [moe_ref.apply_experts(ex[r][0], ex[r][1], r * el) for r in range(p)]
    backs = moe_ref.ref_return(outs, routes, E)
    res = []
    for r in range(p):
        x, cid, w, _ = capped[r]
        out = moe_ref.ref_combine(backs[r], routes[r][1], w, x.shape[0], K)
        assert same_bits(out, moe_ref.direct(x, cid, w, E)), (name, p, C, r)
        assert int((routes[r][1] >= 0).sum()) == sum(info["keep"][r])
        res.append(dict(x=x, ids=info["ids"][r], clipped_ids=cid, w=w, E=E, rows=ex[r][0], expert_counts=ex[r][1],
                        mat=ex[r][3], emat=info["keep"], send=sends[r], slots=routes[r][1], back=backs[r], out=out,
                        keep=info["keep"], clipped=info["clipped"][r], demand=info["demand"]))
    _MEMO[key] = res
    return res


# ---------------------------------------------------------------- the model under a capacity
CAPACITY_FACTOR = 0.5
GRAD_CASE, GRAD_C = "A", 40


class CappedDenseMoE(moe_model_ref.DenseMoE):
    """moe_model_ref.DenseMoE with first-come capacity over the batch as given (the test passes every
    rank's tokens concatenated rank-major): the assignments are walked in (token, k) order with one
    counter per expert, and one past C = max(1, ceil(f * N / E)) contributes nothing."""

    def __init__(self, full, top_k, capacity_factor):
        super().__init__(full, top_k)
        self.capacity_factor = capacity_factor
        self.last_clipped = None

    def forward(self, x):
        import math
        E = self.w1.shape[0]
        probs = torch.softmax((x @ self.router).to(torch.float32), dim=-1)
        w, ids = torch.topk(probs, self.top_k, dim=-1)
        C = max(1, math.ceil(self.capacity_factor * ids.numel() / E))
        (kept,), _, (self.last_clipped,) = clip_ids([ids.cpu()], E, C)
        kept = kept.to(ids.device)
        out = torch.zeros_like(x)
        for k in range(self.top_k):
            for e in range(E):
                m = kept[:, k] == e
                if bool(m.any()):
                    y = torch.relu(x[m] @ self.w1[e] + self.b1[e]) @ self.w2[e] + self.b2[e]
                    out = out.index_put((m.nonzero().view(-1),), w[m, k].unsqueeze(1) * y, accumulate=True)
        return out


def train(comm, device):
    """moe_model_ref.train with ``capacity_factor``: per step (this rank's loss, the single-process
    capped model's loss over every rank's tokens), the drift, and per step this rank's
    (clipped, demand total of the job, capacity) from ``model.last_plan``."""
    from mp4x.models.moe import ExpertParallelMoE
    m = moe_model_ref
    r, p = comm.getRank(), comm.getSlaveNum()
    model = ExpertParallelMoE(comm, m.D_MODEL, m.D_HIDDEN, m.EXPERTS, m.TOP_K, seed=m.SEED, device=device,
                              capacity_factor=CAPACITY_FACTOR)
    ref = CappedDenseMoE(ExpertParallelMoE.init_weights(m.D_MODEL, m.D_HIDDEN, m.EXPERTS, m.SEED), m.TOP_K,
                         CAPACITY_FACTOR).to(device)
    data = [tuple(t.to(device) for t in m.batch(i)) for i in range(p)]
    allx, ally = torch.cat([d[0] for d in data]), torch.cat([d[1] for d in data])
    opt = torch.optim.SGD(model.parameters(), lr=m.LR)
    ropt = torch.optim.SGD(ref.parameters(), lr=m.LR)
    mine, whole, plans = [], [], []
    assert model.last_plan is None
    for _ in range(m.STEPS):
        loss = ((model(data[r][0]) - data[r][1]) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        model.sync_gradients()
        opt.step()
        rloss = ((ref(allx) - ally) ** 2).mean()
        ropt.zero_grad()
        rloss.backward()
        ropt.step()
        mine.append(float(loss.detach()))
        whole.append(float(rloss.detach()))
        plan = model.last_plan
        plans.append(dict(clipped=plan.clipped, demand=sum(sum(row) for row in plan.demand_matrix),
                          kept=sum(sum(row) for row in plan.expert_matrix), capacity=plan.capacity,
                          ref_clipped=ref.last_clipped))
    lo = model.first_expert
    drift = float((model.w2.detach() - ref.w2.detach()[lo:lo + model.local_experts]).abs().max())
    return mine, whole, drift, plans


def check_plans(res, p):
    """``res[r]`` = train()'s result of rank r.  Every step clips: N = p * TOKENS * TOP_K assignments against E * C = E * ceil(f * N / E) places."""
    import math
    m = moe_model_ref
    N = p * m.TOKENS * m.TOP_K
    C = max(1, math.ceil(CAPACITY_FACTOR * N / m.EXPERTS))
    assert (N, C) == (96, 12) and N > m.EXPERTS * C
    for step in range(m.STEPS):
        plans = [res[r][3][step] for r in range(p)]
        clipped = sum(pl["clipped"] for pl in plans)
        for pl in plans:
            assert pl["capacity"] == C and pl["demand"] == N, pl
            assert pl["kept"] == N - clipped <= m.EXPERTS * C, (pl, clipped)
            assert pl["ref_clipped"] == clipped, (pl, clipped)  # the single-process model dropped as many
        assert N - m.EXPERTS * C <= clipped < N, (step, clipped)
        assert 0 < clipped < N, (step, clipped)


def gradients(comm, device):
    """moe_model_ref.gradients under the capacity GRAD_C on case GRAD_CASE: the contract is computed
    from the clipped ids; the calls get the unclipped ids and the capacity."""
    from mp4x.models.moe import combine_tokens, dispatch_tokens
    r, p = comm.getRank(), comm.getSlaveNum()
    capped, routes, info = clipped_case(GRAD_CASE, p, GRAD_C)
    E = capped[0][3]
    K = capped[0][1].shape[1]
    width = capped[0][0].shape[1]
    sends = [moe_ref.ref_send(x, rt[2], K) for (x, _, _, _), rt in zip(capped, routes)]
    ex = moe_ref.ref_exchange(sends, routes, E)
    x, cid, w, _ = capped[r]
    ids = info["ids"][r]
    T = x.shape[0]

    xd = x.to(device).requires_grad_(True)
    rows, plan = dispatch_tokens(comm, xd, ids.to(device), E, capacity=GRAD_C)
    g_rows = [moe_ref.tokens(ex[i][0].shape[0], width, x.dtype, 7100 + i) for i in range(p)]
    rows.backward(g_rows[r].to(device))
    want_gx = moe_ref.ref_combine(moe_ref.ref_return(g_rows, routes, E)[r], routes[r][1], None, T, K)
    ok_dispatch = same_bits(xd.grad, want_gx) if T else xd.grad is None or xd.grad.numel() == 0

    y = [moe_ref.tokens(ex[i][0].shape[0], width, x.dtype, 7200 + i) for i in range(p)]
    g_out = [moe_ref.tokens(capped[i][0].shape[0], width, x.dtype, 7300 + i) for i in range(p)]
    yd = y[r].to(device).requires_grad_(True)
    wd = w.to(device).requires_grad_(True)
    out = combine_tokens(comm, yd, plan, wd)
    out.backward(g_out[r].to(device))
    scaled = [moe_ref.ref_send(g_out[i], routes[i][2], K, capped[i][2]) for i in range(p)]
    want_gy = moe_ref.ref_exchange(scaled, routes, E)[r][0]
    ok_rows = same_bits(yd.grad, want_gy)
    back = moe_ref.ref_return(y, routes, E)[r]
    ok_w, ok_clipped, worst, n_clipped = True, True, 0.0, 0
    if T:
        gw = wd.grad.cpu()
        flat_ids, flat_cid = ids.reshape(-1), cid.reshape(-1)
        for t in range(T):
            for k in range(K):
                s = int(routes[r][1][t * K + k])
                if s < 0:
                    ok_w = ok_w and float(gw[t, k]) == 0.0
                    if int(flat_ids[t * K + k]) >= 0:            # dropped by the capacity, not by the caller
                        assert int(flat_cid[t * K + k]) == -1
                        n_clipped += 1
                        ok_clipped = ok_clipped and float(gw[t, k]) == 0.0
                    continue
                prod = g_out[r][t].to(torch.float64) * back[s].to(torch.float64)
                bound = width * 2.0 ** -24 * float(prod.abs().sum())
                err = abs(float(gw[t, k]) - float(prod.sum()))
                worst = max(worst, err - bound)
                ok_w = ok_w and err <= bound
    want_out = moe_ref.ref_combine(back, routes[r][1], w, T, K)
    return dict(dispatch=ok_dispatch, rows=ok_rows, weights=ok_w, clipped_weights=ok_clipped, n_clipped=n_clipped,
                plan_clipped=plan.clipped, want_clipped=info["clipped"][r], worst=worst,
                out=same_bits(out.detach(), want_out), slots=torch.equal(plan.slots.cpu(), routes[r][1]))
