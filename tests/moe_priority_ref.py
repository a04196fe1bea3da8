"""The definition of the per-expert top-S select (drop by gate weight) in plain Python / numpy: per
expert, ``sorted`` on ``(key, -a)`` with the key made from the ``struct``-packed bits of the float.  No
torch sort: it shares nothing with ``mp4x.parallel.moe.priority_mask_torch`` or the kernels.

Also the case table of the select's tests and the inputs of the dispatch tests."""
import struct

import numpy as np
import torch

import moe_ref

HUGE = 1 << 40


def gate_key(bits):
    """Unsigned order == float order of the float32 with these bits; -0 folded onto +0."""
    if bits & 0x7fffffff == 0:
        bits = 0
    return bits ^ 0xffffffff if bits >> 31 else bits ^ 0x80000000


def float_bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def mask(ids, priority_bits, nb, limit):
    """(out ids as a list, masked): ``ids`` a sequence of ints, ``priority_bits`` the uint32 bit patterns
    of the priorities, ``limit`` an int or a sequence of nb ints (negative: 0)."""
    ids = [int(v) for v in ids]
    out = list(ids)
    per = {}
    for a, e in enumerate(ids):
        if 0 <= e < nb:
            per.setdefault(e, []).append(a)
    masked = 0
    for e, members in per.items():
        lim = int(limit) if isinstance(limit, int) else int(limit[e])
        best_first = sorted(members, key=lambda a: (gate_key(int(priority_bits[a])), -a), reverse=True)
        for a in best_first[max(lim, 0):]:
            out[a] = -1
            masked += 1
    return out, masked


def bits_of(priority):
    """The uint32 bit patterns of a float32 tensor, NaN payloads and signs kept."""
    return priority.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32).reshape(-1)


def from_bits(bits):
    return torch.from_numpy(np.asarray(bits, dtype=np.uint32).view(np.int32).copy()).view(torch.float32)


def mask_tensors(ids, priority, nb, limit):
    """:func:`mask` on tensors: (out in the ids' dtype and shape, masked as an int)."""
    if isinstance(limit, torch.Tensor):
        limit = limit.cpu().tolist()
    out, masked = mask(ids.cpu().reshape(-1).tolist(), bits_of(priority), nb, limit)
    return torch.tensor(out, dtype=ids.dtype).view(ids.shape), masked


def position_mask(ids, nb, limit):
    """The position policy: the first limit[e] assignments of expert e stay."""
    out, seen = [int(v) for v in ids], {}
    for a, e in enumerate(out):
        if 0 <= e < nb:
            lim = int(limit) if isinstance(limit, int) else int(limit[e])
            if seen.get(e, 0) >= lim:
                out[a] = -1
            seen[e] = seen.get(e, 0) + 1
    return out


# ---------------------------------------------------------------- priorities
SPECIAL_BITS = [0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7fffffff, 0xffffffff,
                0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00800000, 0x3f800000, 0xbf800000]


def priorities(kind, n, seed):
    """float32 [n] of one kind: ``constant``; ``lastbit`` (pairs that differ in the last mantissa bit);
    ``special`` (+-0, +-inf, both NaNs, denormals); ``index`` (two values whose keys share their three high
    bytes, so only the last key byte and the index bytes decide); ``random`` (any gate weight in [0, 1))."""
    g = np.random.default_rng(seed)
    if kind == "constant":
        bits = np.full(n, float_bits(0.25), dtype=np.uint32)
    elif kind == "lastbit":
        bits = (0x3f000000 + g.integers(0, 2, n)).astype(np.uint32)
    elif kind == "special":
        bits = np.asarray(SPECIAL_BITS, dtype=np.uint32)[g.integers(0, len(SPECIAL_BITS), n)]
    elif kind == "index":
        bits = (0x3e800000 + 0x80 * g.integers(0, 2, n)).astype(np.uint32)
    else:
        bits = g.random(n, dtype=np.float32).view(np.uint32)
    return from_bits(bits)


KINDS = ("constant", "lastbit", "special", "index", "random")


def ids_for(n, nb, seed, strays=True):
    """int64 [n]: experts drawn from a few hot ones and the whole range, with negative ids and ids >= nb
    mixed in."""
    g = np.random.default_rng(seed)
    hot = g.integers(0, nb, max(1, min(nb, 3)))
    ids = np.where(g.random(n) < 0.6, hot[g.integers(0, len(hot), n)], g.integers(0, nb, n))
    if strays:
        r = g.random(n)
        ids = np.where(r < 0.05, -1 - g.integers(0, 3, n), np.where(r > 0.95, nb + g.integers(0, 3, n), ids))
    return torch.from_numpy(ids.astype(np.int64))


def limit_vector(ids, nb, seed):
    """int64 [nb] holding 0, cnt - 1, cnt, cnt + 1 and a huge value, in turn over the experts in use."""
    cnt = np.bincount(ids.numpy()[(ids.numpy() >= 0) & (ids.numpy() < nb)], minlength=nb)
    lim = np.zeros(nb, dtype=np.int64)
    turn = seed
    for e in range(nb):
        c = int(cnt[e])
        lim[e] = (0, max(c - 1, 0), c, c + 1, HUGE)[turn % 5]
        if c:
            turn += 1
    return torch.from_numpy(lim)


# (n, nb) of the select's table: a tile tail, three tiles; one expert, a few, many, most of them empty
SHAPES = [(111, 1), (111, 3), (111, 64), (600, 1), (600, 3), (600, 64), (600, 2048)]


# ---------------------------------------------------------------- the layer's checks (tiny shapes only)
D_MODEL, D_HIDDEN, TOKENS, TOP_K, MODEL_S = 16, 32, 24, 2, 5


def _grads(layer, x):
    for q in layer.parameters():
        q.grad = None
    out = layer(x)
    out.square().sum().backward()
    return out, [q.grad.clone() for q in (layer.router, layer.w1, layer.b1, layer.w2, layer.b2)]


def model_checks(comm, device):
    """What the model tests assert, as a dict of booleans and counts (rank-local)."""
    from mp4x.models.moe import ExpertParallelMoE, combine_tokens, dispatch_tokens
    r, p = comm.getRank(), comm.getSlaveNum()
    E = 2 * p
    x = (torch.randn(TOKENS, D_MODEL, generator=torch.Generator().manual_seed(300 + r))).to(device)
    res = {}

    def layer(**kw):
        return ExpertParallelMoE(comm, D_MODEL, D_HIDDEN, E, TOP_K, seed=3, device=device, **kw)

    def same(a, b):
        return a.dtype == b.dtype and a.shape == b.shape and bool((a.contiguous().view(torch.int32)
                                                                  == b.contiguous().view(torch.int32)).all())

    # no overflow: "probs" is "position" bit for bit, output and every gradient
    for label, kw in (("share", dict(source_capacity=TOKENS * TOP_K)), ("factor", dict(capacity_factor=float(E)))):
        out0, g0 = _grads(layer(**kw), x)
        out1, g1 = _grads(layer(drop_policy="probs", **kw), x)
        res["no_overflow_" + label] = same(out0, out1) and all(same(a, b) for a, b in zip(g0, g1))
    # overflow: the kept set is the top S of every expert by gate weight
    m = layer(source_capacity=MODEL_S, drop_policy="probs")
    w, ids = m.route(x)
    m(x)
    plan = m.last_plan
    ids_m, masked = mask_tensors(ids, w.detach(), E, MODEL_S)
    pos = position_mask(ids.cpu().reshape(-1).tolist(), E, MODEL_S)
    res["kept_set"] = (plan.slots.cpu() >= 0).tolist() == (ids_m.reshape(-1) >= 0).tolist()
    res["dropped"] = plan.dropped.tolist() == [masked, 0, 0]
    res["n_cut"] = masked
    res["differs"] = ids_m.reshape(-1).tolist() != pos
    # the gate-weight gradient of a dropped assignment is +0 (its bits), through both combine backwards
    for backward in ("torch", "fused"):
        wg = w.detach().clone().contiguous().requires_grad_(True)
        xg = x.clone().requires_grad_(True)
        rows, plan = dispatch_tokens(comm, xg, ids, E, source_capacity=MODEL_S, priority=wg)
        out = combine_tokens(comm, rows * 2, plan, wg, backward=backward)
        out.square().sum().backward()
        gone = (plan.slots < 0).view_as(wg)
        gbits = wg.grad.contiguous().view(torch.int32)
        res["zero_grad_" + backward] = bool((gbits[gone] == 0).all()) and bool((gbits[~gone] != 0).any()) \
            and int(gone.sum()) == masked and xg.grad is not None
    return res


def check_model(res, p):
    for r in range(p):
        row = res[r]
        for key in ("no_overflow_share", "no_overflow_factor", "kept_set", "dropped", "zero_grad_torch",
                    "zero_grad_fused"):
            assert row[key] is True, (r, key, row)
    assert sum(res[r]["n_cut"] for r in range(p)) > 0 and any(res[r]["differs"] for r in range(p))


# ---------------------------------------------------------------- the dispatch tests' inputs
# name -> (T, K, experts per rank, width, share S, capacity C): every expert in reach overflows somewhere
DISPATCH = {"small": (37, 3, 2, 4, 9, 40), "ties": (64, 2, 1, 8, 20, 70)}


def dispatch_case(name, r, p):
    """(x, ids, w, E) of rank r: gate weights in sixteenths, so many equal priorities."""
    T, K, el, width, _, _ = DISPATCH[name]
    E = el * p
    g = torch.Generator().manual_seed(9100 + 10 * len(name) + r)
    ids = torch.randint(0, E, (T, K), generator=g)
    ids[torch.rand(T, K, generator=g) < 0.08] = -1
    x = moe_ref.tokens(T, width, torch.float32, 9200 + r)
    w = moe_ref.gate_weights(T, K, 9300 + 10 * len(name) + r)
    return x, ids, w, E
