"""The contract of the expert-parallel token dispatch / combine (dispatchTokens / combineTokens and
the K9 kernels under them) in plain torch on the CPU, and the cases the tests run.  Shared by
tests/test_moe_cpu.py, tests/test_moe_kernels_gpu.py, tests/test_moe_api_gpu.py and the model tests.

With a = t*K + k the flattened assignments of one rank and E experts, rank r of p owning experts
[r*E/p, (r+1)*E/p):

    slots      the stable sort of the assignments by expert id; ids < 0 or >= E get slot -1
    send       send[slots[a]] = x[a // K]  (times row_scale[a] in f32, one rounding, when given)
    dispatch   rank r receives, from every source i in rank order, i's send rows of r's experts;
               regrouped expert-major: by local expert, then source rank, then sender order
    return     the inverse: every row back on its sender at its slot
    combine    out[t] = round(acc), acc = +0.0f, then for k = 0..K-1 with slots[t*K+k] >= 0:
               acc = acc + w[t, k] * f32(back[slots[t*K+k]])   (eager torch: two roundings)

Token values are multiples of 1/8 in [-8, 8) and weights multiples of 1/16 in (0, 1), drawn from
per-rank seeded generators, and the "experts" of the API tests multiply by a small integer, so every
product and sum is exact in f32 and every comparison is bit for bit.
"""
import torch

from fp8_rsag_ref import bits, same_bits  # noqa: F401  (re-exported for the tests)

MAX_EXPERTS = 2048


# ---------------------------------------------------------------- the contract
def ref_route(ids, E):
    """(counts int64[E + 2], slots int64[n], order): order[s] = the assignment at slot s."""
    ids = ids.reshape(-1).to(torch.int64)
    placed = (ids >= 0) & (ids < E)
    key = torch.where(placed, ids, torch.full_like(ids, E))
    order = torch.sort(key, stable=True).indices[:int(placed.sum())]
    slots = torch.full((ids.numel(),), -1, dtype=torch.int64)
    slots[order] = torch.arange(order.numel())
    counts = torch.tensor([int((ids == e).sum()) for e in range(E)] + [int((ids < 0).sum()), int((ids >= E).sum())],
                          dtype=torch.int64)
    return counts, slots, order


def ref_send(x, order, K, row_scale=None):
    rows = x[order // K]
    if row_scale is None:
        return rows.clone()
    s = row_scale.reshape(-1)[order].to(torch.float32).view((-1,) + (1,) * (x.dim() - 1))
    return (s * rows.to(torch.float32)).to(x.dtype)


def ref_combine(back, slots, weights, T, K):
    out = torch.zeros((T,) + tuple(back.shape[1:]), dtype=torch.float32)
    for t in range(T):
        acc = torch.zeros(tuple(back.shape[1:]), dtype=torch.float32)
        for k in range(K):
            s = int(slots[t * K + k])
            if s < 0:
                continue
            w = weights.reshape(-1)[t * K + k] if weights is not None else torch.tensor(1.0)
            acc = acc + w * back[s].to(torch.float32)
        out[t] = acc
    return out.to(back.dtype)


def ref_exchange(sends, routes, E):
    """Per rank: (rows expert-major, expert_counts, source-major rows, the rank count matrix).
    ``sends[i]`` are rank i's send rows, ``routes[i]`` its ref_route result."""
    p = len(sends)
    el = E // p
    cnt = [r[0][:E].tolist() for r in routes]
    mat = [[sum(cnt[i][j * el:(j + 1) * el]) for j in range(p)] for i in range(p)]
    out = []
    for r in range(p):
        seg = {}
        for i in range(p):
            off = sum(cnt[i][:r * el])
            for e in range(el):
                c = cnt[i][r * el + e]
                seg[(i, e)] = sends[i][off:off + c]
                off += c
        source_major = torch.cat([seg[(i, e)] for i in range(p) for e in range(el)])
        expert_major = torch.cat([seg[(i, e)] for e in range(el) for i in range(p)])
        out.append((expert_major, [sum(cnt[i][r * el + e] for i in range(p)) for e in range(el)], source_major, mat))
    return out


def ref_return(expert_rows, routes, E):
    """The inverse of ref_exchange: per rank, its rows back in slot order.  ``expert_rows[r]`` in
    rank r's expert-major layout."""
    p = len(expert_rows)
    el = E // p
    cnt = [r[0][:E].tolist() for r in routes]
    pieces = {}
    for r in range(p):
        off = 0
        for e in range(el):
            for i in range(p):
                c = cnt[i][r * el + e]
                pieces[(i, r * el + e)] = expert_rows[r][off:off + c]
                off += c
    return [torch.cat([pieces[(i, g)] for g in range(E)]) for i in range(p)]


def expert_factor(e):
    """The integer "expert" of the API tests: expert e multiplies its rows by this."""
    return e % 3 + 1


def apply_experts(rows, expert_counts, first_expert):
    out, off = rows.clone(), 0
    for e, c in enumerate(expert_counts):
        out[off:off + c] = (rows[off:off + c].to(torch.float32) * expert_factor(first_expert + e)).to(rows.dtype)
        off += c
    return out


def direct(x, ids, weights, E):
    """dispatch -> integer experts -> combine, per token, with no routing at all."""
    T = x.shape[0]
    ids2 = ids.reshape(T, ids.numel() // max(T, 1))
    out = torch.zeros_like(x)
    for t in range(T):
        acc = torch.zeros(tuple(x.shape[1:]), dtype=torch.float32)
        for k in range(ids2.shape[1]):
            e = int(ids2[t, k])
            if e < 0:
                continue
            y = (x[t].to(torch.float32) * expert_factor(e)).to(x.dtype)
            w = weights.reshape(T, ids2.shape[1])[t, k] if weights is not None else torch.tensor(1.0)
            acc = acc + w * y.to(torch.float32)
        out[t] = acc.to(x.dtype)
    return out


# ---------------------------------------------------------------- the cases
def tokens(T, width, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-64, 64, (T, width), generator=g).to(torch.float32) / 8).to(dtype)


def gate_weights(T, K, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(1, 16, (T, K), generator=g).to(torch.float32) / 16


# name -> (T, K, experts per rank, dtype name, width, id dtype name)
CASES = {
    "A": (173, 3, 4, "float32", 4, "int64"),
    "B": (5, 2, 1, "bfloat16", 24, "int32"),
    "C": (300, 1, 32, "float16", 8, "int32"),
    "D": (130, 2, 2, "float32", 260, "int64"),
}
# case D's shape with the fp8 wire codec: bf16 rows of V = 65 vectors (520 elements; 260 bf16 would
# be 520 bytes, no whole number of 16-byte vectors)
FP8_CASE = (130, 2, 2, "bfloat16", 520, "int64")


def case_ids(name, r, p):
    T, K, el, _, _, idt = CASES[name] if name in CASES else FP8_CASE
    E = el * p
    if name == "A":
        if r == 1:
            T = 0
        g = torch.Generator().manual_seed(4100 + r)
        ids = torch.randint(0, E - 1, (T, K), generator=g)
        ids = ids + (ids >= 1).to(ids.dtype)                     # expert 1 is chosen by nobody
        ids[torch.rand(T, K, generator=g) < 0.1] = -1
        if T:
            ids[0] = -1                                          # token 0 wholly dropped
    elif name == "B":
        g = torch.Generator().manual_seed(4200 + r)
        ids = torch.randint(0, E, (T, 1), generator=g).expand(T, 2).contiguous()
    elif name == "C":
        ids = ((7 * torch.arange(T * K) + r) % E).view(T, K)
    else:                                                        # D and its fp8 form
        ids = torch.full((T, K), E - 1)
    return ids.to(getattr(torch, idt))


def case(name, r, p):
    """(x [T, width], ids [T, K], weights [T, K], E) of rank r; asserts the case's properties."""
    T, K, el, dt, width, _ = CASES[name] if name in CASES else FP8_CASE
    E = el * p
    ids = case_ids(name, r, p)
    T = ids.shape[0]
    x = tokens(T, width, getattr(torch, dt), 5000 + 10 * ord(name[0]) + r)
    w = gate_weights(T, K, 6000 + 10 * ord(name[0]) + r)
    assert x.numel() == 0 or (float(x.float().abs().max()) <= 8 and bool(((x.float() * 8) % 1 == 0).all()))
    assert w.numel() == 0 or (0 < float(w.min()) and float(w.max()) < 1 and bool(((w * 16) % 1 == 0).all()))
    return x, ids, w, E


def check_case_properties(name, p):
    """What each case is for, asserted on its inputs (every rank's)."""
    per_rank = [case(name, r, p) for r in range(p)]
    E = per_rank[0][3]
    el = E // p
    routes = [ref_route(ids, E) for _, ids, _, _ in per_rank]
    cnt = [rt[0] for rt in routes]
    if name == "A":
        assert per_rank[0][1].numel() == 519 == 2 * 256 + 7
        assert p == 1 or per_rank[1][1].numel() == 0                         # an empty rank
        assert all(int(c[1]) == 0 for c in cnt)                              # an empty expert
        assert all(int(c[E]) > 0 for i, c in enumerate(cnt) if i != 1)       # dropped assignments
        assert all(int(c[E + 1]) == 0 for c in cnt)
        assert bool((per_rank[0][1][0] < 0).all())                           # a zero output row
        assert per_rank[0][1].dtype == torch.int64
        assert any(int(c[e]) == 0 for c in cnt for e in range(E))            # empty (source, expert) segments
    elif name == "B":
        assert el == 1 and per_rank[0][1].numel() == 10 < 64
        assert all(bool((ids[:, 0] == ids[:, 1]).all()) for _, ids, _, _ in per_rank)
        assert per_rank[0][0].shape[1] * 2 == 48                             # V = 3
    elif name == "C" and p > 1:
        assert E in (64, 96)
        for _, ids, _, _ in per_rank:
            flat = ids.reshape(-1)
            for w0 in range(0, 256, 64):
                assert flat[w0:w0 + 64].unique().numel() == 64              # 64 distinct experts per full wave
    elif name != "C":
        assert all(bool((ids == E - 1).all()) for _, ids, _, _ in per_rank)
        assert per_rank[0][1].numel() == 260 > 256
        assert per_rank[0][0].shape[1] * per_rank[0][0].element_size() == 65 * 16
    return per_rank, routes


def end_to_end(name, p):
    """Per rank: dict(rows, expert_counts, slots, counts, out) of the whole contract, checked against
    the direct per-token formula."""
    per_rank, routes = check_case_properties(name, p)
    E = per_rank[0][3]
    el = E // p
    K = per_rank[0][1].shape[1]
    sends = [ref_send(x, rt[2], K) for (x, _, _, _), rt in zip(per_rank, routes)]
    ex = ref_exchange(sends, routes, E)
    outs = [apply_experts(ex[r][0], ex[r][1], r * el) for r in range(p)]
    backs = ref_return(outs, routes, E)
    res = []
    for r in range(p):
        x, ids, w, _ = per_rank[r]
        out = ref_combine(backs[r], routes[r][1], w, x.shape[0], K)
        assert same_bits(out, direct(x, ids, w, E)), (name, p, r)
        res.append(dict(x=x, ids=ids, w=w, E=E, rows=ex[r][0], expert_counts=ex[r][1], source_major=ex[r][2],
                        mat=ex[r][3], send=sends[r], slots=routes[r][1], counts=routes[r][0], back=backs[r], out=out))
    return res
