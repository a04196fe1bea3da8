"""What tests/test_moe_model.py (CPU, gloo) and tests/test_moe_model_gpu.py share: a single-process
mixture-of-experts model in plain torch that holds ALL experts (no routing, no collectives), and the
rank functions that train ``ExpertParallelMoE`` next to it and take the autograd functions' gradients
next to the contract of tests/moe_ref.py."""
import torch

import moe_ref
from moe_ref import same_bits

D_MODEL, D_HIDDEN, EXPERTS, TOP_K, TOKENS, STEPS, SEED, LR = 16, 32, 4, 2, 24, 5, 11, 0.05


class DenseMoE(torch.nn.Module):
    """Every expert in one process: out[t] = sum over k, in k order, of gate[t, k] * mlp_e(x[t])."""

    def __init__(self, full, top_k):
        super().__init__()
        self.top_k = top_k
        for name, t in full.items():
            setattr(self, name, torch.nn.Parameter(t.clone()))

    def forward(self, x):
        probs = torch.softmax((x @ self.router).to(torch.float32), dim=-1)
        w, ids = torch.topk(probs, self.top_k, dim=-1)
        out = torch.zeros_like(x)
        for k in range(self.top_k):
            for e in range(self.w1.shape[0]):
                m = ids[:, k] == e
                if bool(m.any()):
                    y = torch.relu(x[m] @ self.w1[e] + self.b1[e]) @ self.w2[e] + self.b2[e]
                    out = out.index_put((m.nonzero().view(-1),), w[m, k].unsqueeze(1) * y, accumulate=True)
        return out


def batch(rank):
    g = torch.Generator().manual_seed(900 + rank)
    return torch.randn(TOKENS, D_MODEL, generator=g), torch.randn(TOKENS, D_MODEL, generator=g)


def train(comm, device):
    """Per-step (this rank's loss, the single-process model's loss over every rank's tokens)."""
    from mp4x.models.moe import ExpertParallelMoE
    r, p = comm.getRank(), comm.getSlaveNum()
    model = ExpertParallelMoE(comm, D_MODEL, D_HIDDEN, EXPERTS, TOP_K, seed=SEED, device=device)
    ref = DenseMoE(ExpertParallelMoE.init_weights(D_MODEL, D_HIDDEN, EXPERTS, SEED), TOP_K).to(device)
    data = [tuple(t.to(device) for t in batch(i)) for i in range(p)]
    allx, ally = torch.cat([d[0] for d in data]), torch.cat([d[1] for d in data])
    opt = torch.optim.SGD(model.parameters(), lr=LR)
    ropt = torch.optim.SGD(ref.parameters(), lr=LR)
    mine, whole = [], []
    for _ in range(STEPS):
        loss = ((model(data[r][0]) - data[r][1]) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        model.sync_gradients()
        opt.step()
        rloss = ((ref(allx) - ally) ** 2).mean()                 # = the mean over ranks of their losses
        ropt.zero_grad()
        rloss.backward()
        ropt.step()
        mine.append(float(loss))
        whole.append(float(rloss))
    # the experts this rank holds ended where the single-process model's did
    lo = model.first_expert
    drift = float((model.w2.detach() - ref.w2.detach()[lo:lo + model.local_experts]).abs().max())
    return mine, whole, drift


def gradients(comm, device):
    """The two autograd functions' backward passes on exact-valued inputs, against the contract."""
    from mp4x.models.moe import combine_tokens, dispatch_tokens
    r, p = comm.getRank(), comm.getSlaveNum()
    name = "A"
    per_rank, routes = moe_ref.check_case_properties(name, p)
    E = per_rank[0][3]
    K = per_rank[0][1].shape[1]
    el = E // p
    width = per_rank[0][0].shape[1]
    sends = [moe_ref.ref_send(x, rt[2], K) for (x, _, _, _), rt in zip(per_rank, routes)]
    ex = moe_ref.ref_exchange(sends, routes, E)
    x, ids, w, _ = per_rank[r]
    T = x.shape[0]

    # dispatch backward: a combine with unit weights of the rows' gradients on the return path
    xd = x.to(device).requires_grad_(True)
    rows, plan = dispatch_tokens(comm, xd, ids.to(device), E)
    g_rows = [moe_ref.tokens(ex[i][0].shape[0], width, x.dtype, 7100 + i) for i in range(p)]
    rows.backward(g_rows[r].to(device))
    want_gx = moe_ref.ref_combine(moe_ref.ref_return(g_rows, routes, E)[r], routes[r][1], None, T, K)
    ok_dispatch = same_bits(xd.grad, want_gx) if T else xd.grad is None or xd.grad.numel() == 0

    # combine backward w.r.t. the rows: a dispatch of the output's gradient, rows scaled by the gates;
    # w.r.t. the weights: the row dot, against a float64 dot within H * 2^-24 * sum |g * y|
    y = [moe_ref.tokens(ex[i][0].shape[0], width, x.dtype, 7200 + i) for i in range(p)]
    g_out = [moe_ref.tokens(per_rank[i][0].shape[0], width, x.dtype, 7300 + i) for i in range(p)]
    yd = y[r].to(device).requires_grad_(True)
    wd = w.to(device).requires_grad_(True)
    out = combine_tokens(comm, yd, plan, wd)
    out.backward(g_out[r].to(device))
    scaled = [moe_ref.ref_send(g_out[i], routes[i][2], K, per_rank[i][2]) for i in range(p)]
    want_gy = moe_ref.ref_exchange(scaled, routes, E)[r][0]
    ok_rows = same_bits(yd.grad, want_gy)
    back = moe_ref.ref_return(y, routes, E)[r]
    ok_w, worst = True, 0.0
    if T:
        gw = wd.grad.cpu()
        for t in range(T):
            for k in range(K):
                s = int(routes[r][1][t * K + k])
                if s < 0:
                    ok_w = ok_w and float(gw[t, k]) == 0.0
                    continue
                prod = g_out[r][t].to(torch.float64) * back[s].to(torch.float64)
                bound = width * 2.0 ** -24 * float(prod.abs().sum())
                err = abs(float(gw[t, k]) - float(prod.sum()))
                worst = max(worst, err - bound)
                ok_w = ok_w and err <= bound
    want_out = moe_ref.ref_combine(back, routes[r][1], w, T, K)
    return dict(dispatch=ok_dispatch, rows=ok_rows, weights=ok_w, worst=worst, out=same_bits(out.detach(), want_out),
                el=el)
