"""The padded fixed-capacity layout of dispatchTokens (sourceCapacity=S) in plain torch on the CPU,
written from the definition, and the (case, S) pairs the padded tests run.  Shared by
tests/test_moe_padded_cpu.py, the padded kernel / API tests on the GPU and the padded model tests.

Every rank walks its own flattened assignments a = t*K + k in order with one counter per expert: an
assignment with expert e in [0, E) is kept while e's counter on THAT rank is below S, at row
e*S + counter of the rank's send buffer [E*S, ...]; every row nobody was put in is zero.  Rank r
receives, from every source i, the block of its el = E/p experts and holds rows[e, i*S + j] = source
i's row (r*el + e)*S + j.  A cut assignment's id becomes -1; with those ids tests/moe_ref.py gives the
expected output unchanged (a padded call IS the uncapped call on the cut ids).
"""
import torch

import moe_ref
from moe_ref import same_bits  # noqa: F401  (re-exported for the tests)

NO_CUT = 1 << 10             # above every case's per-rank demand (and E * S stays small)

# (case of moe_ref.CASES, S) -> rows every rank keeps, by rank count; asserted by cut_case(), so a case
# cannot silently stop cutting
KEPT = {
    ("A", 40): {2: [280, 0], 3: [431, 0, 433]},       # some experts cut, others not; an empty expert; an empty rank
    ("A", 1): {2: [7, 0], 3: [11, 0, 11]},            # one row per expert
    ("B", 3): {2: [6, 6], 3: [7, 5, 6]},              # one local expert, no regroup; cut inside the first wave
    ("C", 3): {2: [192, 192], 3: [288, 288, 288]},    # 64 distinct experts per wave, every one cut
    ("C", 5): {2: [300, 300], 3: [300, 300, 300]},    # nothing cut, pads only
    ("D", 100): {2: [100, 100], 3: [100, 100, 100]},  # V = 65, tiles split; E * S > T * K
    ("D", 258): {2: [258, 258], 3: [258, 258, 258]},  # cut two rows into the second tile
    ("D", 300): {2: [260, 260], 3: [260, 260, 260]},  # nothing cut, 40 pad rows of 65 vectors
}
NOTHING_CUT = {("C", 5), ("D", 300)}
TABLE = sorted(KEPT)


def cut_ids(ids, E, S):
    """One rank: (the ids with every cut assignment set to -1, slots int64[n], kept[E], dropped[3])."""
    flat = ids.reshape(-1).to(torch.int64).clone()
    slots = torch.full((flat.numel(),), -1, dtype=torch.int64)
    count, over, neg, big = [0] * E, 0, 0, 0
    for a in range(flat.numel()):
        e = int(flat[a])
        if e < 0:
            neg += 1
        elif e >= E:
            big += 1
            flat[a] = -1
        elif count[e] < S:
            slots[a] = e * S + count[e]
            count[e] += 1
        else:
            over += 1
            flat[a] = -1
    return flat.view(ids.shape).to(ids.dtype), slots, count, [over, neg, big]


def send_buffer(x, slots, K, E, S, row_scale=None):
    """[E*S, ...]: row slots[a] = x[a // K] (times row_scale[a], f32, one rounding), zeros elsewhere."""
    out = torch.zeros((E * S,) + tuple(x.shape[1:]), dtype=x.dtype)
    for a in range(slots.numel()):
        s = int(slots[a])
        if s < 0:
            continue
        row = x[a // K]
        if row_scale is not None:
            row = (row_scale.reshape(-1)[a].to(torch.float32) * row.to(torch.float32)).to(x.dtype)
        out[s] = row
    return out


def exchange(sends, E, S):
    """Per rank r: rows [el, p*S, ...], rows[e, i*S + j] = sends[i][(r*el + e)*S + j]."""
    p = len(sends)
    el = E // p
    out = []
    for r in range(p):
        rows = torch.zeros((el, p * S) + tuple(sends[0].shape[1:]), dtype=sends[0].dtype)
        for e in range(el):
            for i in range(p):
                rows[e, i * S:(i + 1) * S] = sends[i][(r * el + e) * S:(r * el + e + 1) * S]
        out.append(rows)
    return out


def give_back(expert_rows, E, S):
    """The inverse of exchange: per rank i, [E*S, ...] in slot order."""
    p = len(expert_rows)
    el = E // p
    out = []
    for i in range(p):
        back = torch.zeros((E * S,) + tuple(expert_rows[0].shape[2:]), dtype=expert_rows[0].dtype)
        for r in range(p):
            for e in range(el):
                back[(r * el + e) * S:(r * el + e + 1) * S] = expert_rows[r][e, i * S:(i + 1) * S]
        out.append(back)
    return out


def apply_experts(rows, first_expert):
    """The integer experts of moe_ref on the padded layout [el, p*S, ...] (pads stay zero)."""
    out = rows.clone()
    for e in range(rows.shape[0]):
        out[e] = (rows[e].to(torch.float32) * moe_ref.expert_factor(first_expert + e)).to(rows.dtype)
    return out


def pads_are_zero_bits(rows, valid, S):
    """Every row of rows [el, p*S, ...] past its source's valid count is all-zero BITS (+0)."""
    el, p = valid.shape
    flat = moe_ref.bits(rows).reshape(el, p, S, -1)
    for e in range(el):
        for i in range(p):
            if bool((flat[e, i, int(valid[e, i]):] != 0).any()):
                return False
    return True


def from_inputs(per_rank, S):
    """The whole contract for per-rank (x, ids, w, E): per rank a dict of everything expected."""
    p = len(per_rank)
    E = per_rank[0][3]
    el = E // p
    cuts = [cut_ids(ids, E, S) for _, ids, _, _ in per_rank]
    K = [ids.shape[1] if ids.dim() == 2 else 1 for _, ids, _, _ in per_rank]
    sends = [send_buffer(x, c[1], k, E, S) for (x, _, _, _), c, k in zip(per_rank, cuts, K)]
    rows = exchange(sends, E, S)
    backs = give_back([apply_experts(rows[r], r * el) for r in range(p)], E, S)
    res = []
    for r in range(p):
        x, ids, w, _ = per_rank[r]
        cids, slots, kept, dropped = cuts[r]
        out = moe_ref.ref_combine(backs[r], slots, w, x.shape[0], K[r])
        assert same_bits(out, moe_ref.direct(x, cids, w, E)), (p, r, S)        # the equivalence itself
        valid = torch.tensor([[cuts[i][2][r * el + e] for i in range(p)] for e in range(el)], dtype=torch.int64)
        assert pads_are_zero_bits(rows[r], valid, S)
        res.append(dict(x=x, ids=ids, w=w, E=E, S=S, K=K[r], cut_ids=cids, slots=slots, send=sends[r], rows=rows[r],
                        kept=torch.tensor(kept, dtype=torch.int64), valid=valid,
                        dropped=torch.tensor(dropped, dtype=torch.int64), back=backs[r], out=out))
    return res


_MEMO = {}


def end_to_end(name, p, S):
    """Per rank: the expected result of case ``name`` with share S; the table's kept rows asserted."""
    key = (name, p, S)
    if key not in _MEMO:
        per_rank, _ = moe_ref.check_case_properties(name, p)
        res = from_inputs(per_rank, S)
        kept = [int(d["kept"].sum()) for d in res]
        cut = sum(int(d["dropped"][0]) for d in res)
        if (name, S) in KEPT and p in KEPT[(name, S)]:
            assert kept == KEPT[(name, S)][p], (name, S, p, kept)
            assert (cut == 0) == ((name, S) in NOTHING_CUT), (name, S, p, cut)
        if S == NO_CUT:
            assert cut == 0
        _MEMO[key] = res
    return _MEMO[key]


# ---------------------------------------------------------------- the model under a per-source share
MODEL_S = 10                 # 24 tokens x top-2 = 48 assignments per rank over 4 experts: some expert is cut
GRAD_CASE, GRAD_S = "A", 40


def _dense_model(full, top_k, S):
    import moe_model_ref

    class PaddedDenseMoE(moe_model_ref.DenseMoE):
        """moe_model_ref.DenseMoE with per-source first-come: ``forward`` takes the per-rank batches; each
        rank's assignments are walked in (token, k) order with one counter per (rank, expert), and one
        past S contributes nothing."""

        def __init__(self):
            super().__init__(full, top_k)
            self.last_cut = None

        def forward(self, batches):
            E = self.w1.shape[0]
            outs, self.last_cut = [], []
            for x in batches:
                probs = torch.softmax((x @ self.router).to(torch.float32), dim=-1)
                w, ids = torch.topk(probs, self.top_k, dim=-1)
                kept, _, _, dropped = cut_ids(ids.cpu(), E, S)
                kept = kept.to(ids.device)
                self.last_cut.append(dropped[0])
                out = torch.zeros_like(x)
                for k in range(self.top_k):
                    for e in range(E):
                        m = kept[:, k] == e
                        if bool(m.any()):
                            y = torch.relu(x[m] @ self.w1[e] + self.b1[e]) @ self.w2[e] + self.b2[e]
                            out = out.index_put((m.nonzero().view(-1),), w[m, k].unsqueeze(1) * y, accumulate=True)
                outs.append(out)
            return torch.cat(outs)

    return PaddedDenseMoE()


def train(comm, device):
    """moe_model_ref.train with ``source_capacity``: per step (this rank's loss, the single-process
    per-source first-come model's loss over every rank's batch), the drift, and per step this rank's
    cut assignments from ``model.last_plan.dropped`` next to the dense model's for this rank."""
    import moe_model_ref as m
    from mp4x.models.moe import ExpertParallelMoE
    r, p = comm.getRank(), comm.getSlaveNum()
    model = ExpertParallelMoE(comm, m.D_MODEL, m.D_HIDDEN, m.EXPERTS, m.TOP_K, seed=m.SEED, device=device,
                              source_capacity=MODEL_S)
    ref = _dense_model(ExpertParallelMoE.init_weights(m.D_MODEL, m.D_HIDDEN, m.EXPERTS, m.SEED), m.TOP_K,
                       MODEL_S).to(device)
    data = [tuple(t.to(device) for t in m.batch(i)) for i in range(p)]
    ally = torch.cat([d[1] for d in data])
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
        rloss = ((ref([d[0] for d in data]) - ally) ** 2).mean()
        ropt.zero_grad()
        rloss.backward()
        ropt.step()
        mine.append(float(loss.detach()))
        whole.append(float(rloss.detach()))
        plan = model.last_plan
        el = m.EXPERTS // p
        plans.append(dict(cut=int(plan.dropped[0]), ref_cut=ref.last_cut[r], S=plan.source_capacity,
                          rows=tuple(plan.expert_counts) == (p * MODEL_S,) * el,
                          kept=int(plan.kept.sum()), valid=int(plan.valid.sum())))
    lo = model.first_expert
    drift = float((model.w2.detach() - ref.w2.detach()[lo:lo + model.local_experts]).abs().max())
    return mine, whole, drift, plans


def check_plans(res, p):
    """``res[r]`` = train()'s result of rank r: every step's cut equals the dense model's, something is
    cut, and what the ranks kept is what the experts were told is valid."""
    import moe_model_ref as m
    assert m.TOKENS * m.TOP_K > m.EXPERTS * MODEL_S                # a rank cannot keep everything
    for step in range(m.STEPS):
        plans = [res[r][3][step] for r in range(p)]
        for pl in plans:
            assert pl["S"] == MODEL_S and pl["rows"] and pl["cut"] == pl["ref_cut"] > 0, pl
            assert pl["kept"] == m.TOKENS * m.TOP_K - pl["cut"], pl
        assert sum(pl["kept"] for pl in plans) == sum(pl["valid"] for pl in plans), plans


def gradients(comm, device):
    """moe_model_ref.gradients under the share GRAD_S on case GRAD_CASE, in the padded layout: the
    dispatch's backward against the unit-weight combine of the returned gradient rows, the combine's
    backward w.r.t. the rows against the padded scatter scaled by the gates (pads zero), both bit for
    bit; w.r.t. the weights against a float64 dot, exactly 0 for a cut assignment."""
    from mp4x.models.moe import combine_tokens, dispatch_tokens
    r, p = comm.getRank(), comm.getSlaveNum()
    res = end_to_end(GRAD_CASE, p, GRAD_S)
    E, S = res[0]["E"], GRAD_S
    el = E // p
    K = res[0]["K"]
    width = res[0]["x"].shape[1]
    x, ids, w, slots = res[r]["x"], res[r]["ids"], res[r]["w"], res[r]["slots"]
    T = x.shape[0]
    rnd = lambda seed: moe_ref.tokens(el * p * S, width, x.dtype, seed).view(el, p * S, width)   # noqa: E731

    xd = x.to(device).requires_grad_(True)
    rows, plan = dispatch_tokens(comm, xd, ids.to(device), E, source_capacity=S)
    g_rows = [rnd(7100 + i) for i in range(p)]                    # nonzero on the pad rows too: never read
    rows.backward(g_rows[r].to(device))
    want_gx = moe_ref.ref_combine(give_back(g_rows, E, S)[r], slots, None, T, K)
    ok_dispatch = same_bits(xd.grad, want_gx) if T else xd.grad is None or xd.grad.numel() == 0

    y = [rnd(7200 + i) for i in range(p)]
    g_out = [moe_ref.tokens(res[i]["x"].shape[0], width, x.dtype, 7300 + i) for i in range(p)]
    yd = y[r].to(device).requires_grad_(True)
    wd = w.to(device).requires_grad_(True)
    out = combine_tokens(comm, yd, plan, wd)
    out.backward(g_out[r].to(device))
    scaled = [send_buffer(g_out[i], res[i]["slots"], K, E, S, res[i]["w"]) for i in range(p)]
    want_gy = exchange(scaled, E, S)[r]
    ok_rows = same_bits(yd.grad, want_gy) and pads_are_zero_bits(yd.grad.cpu(), res[r]["valid"], S)
    back = give_back(y, E, S)[r]
    ok_w, ok_cut, worst, n_cut = True, True, 0.0, 0
    if T:
        gw = wd.grad.cpu()
        flat_ids = ids.reshape(-1)
        for t in range(T):
            for k in range(K):
                s = int(slots[t * K + k])
                if s < 0:
                    ok_w = ok_w and float(gw[t, k]) == 0.0
                    if int(flat_ids[t * K + k]) >= 0:            # cut by the share, not dropped by the caller
                        n_cut += 1
                        ok_cut = ok_cut and float(gw[t, k]) == 0.0
                    continue
                prod = g_out[r][t].to(torch.float64) * back[s].to(torch.float64)
                bound = width * 2.0 ** -24 * float(prod.abs().sum())
                err = abs(float(gw[t, k]) - float(prod.sum()))
                worst = max(worst, err - bound)
                ok_w = ok_w and err <= bound
    want_out = moe_ref.ref_combine(back, slots, w, T, K)
    return dict(dispatch=ok_dispatch, rows=ok_rows, weights=ok_w, cut_weights=ok_cut, n_cut=n_cut,
                plan_cut=int(plan.dropped[0]), want_cut=int(res[r]["dropped"][0]), worst=worst,
                out=same_bits(out.detach(), want_out), slots=torch.equal(plan.slots.cpu(), slots))
