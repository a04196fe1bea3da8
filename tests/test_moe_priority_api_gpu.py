"""dispatchTokens(..., priority=) / combineTokens through the public API on the GPU (p processes
sharing cuda:0): the padded and the capped ragged call, dispatch -> integer "experts" -> combine with
``priority=w``, bit for bit against the plain call on the ids masked by the plain-Python definition
(tests/moe_priority_ref.py).  The padded call exchanges no counts and makes one copy plan, as the
position call does.  Captured: the padded step recorded once by ``comm.device.capture`` and replayed on
fresh tokens, ids and priorities; every replay equals its eager result."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import moe_priority_ref as ref  # noqa: E402
import moe_ref  # noqa: E402
from moe_ref import same_bits  # noqa: E402
from spawn_ranks import run_spawn  # noqa: E402

pytestmark = pytest.mark.gpu

IPC = ("all_to_all_v.ipc", "all_to_all_v.ipc.padded")


def _moved(stats, before):
    return {k: c - before.get(k, 0) for k, c in stats.items() if c != before.get(k, 0)}


def _factors(first_expert, el):
    return torch.tensor([moe_ref.expert_factor(first_expert + e) for e in range(el)], dtype=torch.float32, device="cuda")


def _padded_experts(rows, factors):
    return (rows.to(torch.float32) * factors.view((-1,) + (1,) * (rows.dim() - 1))).to(rows.dtype)


def _ragged_experts(rows, counts, factors):
    reps = torch.repeat_interleave(factors, torch.tensor(counts, device=rows.device))
    return (rows.to(torch.float32) * reps.view((-1,) + (1,) * (rows.dim() - 1))).to(rows.dtype)


def _api(comm, padded):
    from mp4x.parallel import sparse
    from mp4x.parallel.moe import capacity_quota
    r, p = comm.getRank(), comm.getSlaveNum()
    stats = comm.device.stats
    out = []
    for name in sorted(ref.DISPATCH):
        T, K, el, width, S, C = ref.DISPATCH[name]
        per_rank = [ref.dispatch_case(name, i, p) for i in range(p)]
        x, ids, w, E = per_rank[r]
        counts = [np.bincount(i.reshape(-1).numpy()[i.reshape(-1).numpy() >= 0], minlength=E).tolist()
                  for _, i, _, _ in per_rank]
        limit = S if padded else list(capacity_quota(counts, C)[r])
        kw = dict(sourceCapacity=S) if padded else dict(capacity=C)
        plain_kw = dict(sourceCapacity=S) if padded else {}
        ids_m, masked = ref.mask_tensors(ids, w, E, limit)
        xd, idd, wd, idm = x.to("cuda"), ids.to("cuda"), w.to("cuda"), ids_m.to("cuda")
        factors = _factors(r * el, el)
        gathers, gather = [], sparse._count_matrix
        sparse._count_matrix = lambda *a: gathers.append(1) or gather(*a)
        try:
            before = dict(stats)
            rows, plan = comm.dispatchTokens(xd, idd, E, priority=wd, **kw)
            torch.cuda.synchronize()
            used, exchanged = _moved(stats, before), len(gathers)
        finally:
            sparse._count_matrix = gather
        rows0, plan0 = comm.dispatchTokens(xd, idm, E, **plain_kw)
        if padded:
            y, y0 = _padded_experts(rows, factors), _padded_experts(rows0, factors)
        else:
            y = _ragged_experts(rows, plan.expert_counts, factors)
            y0 = _ragged_experts(rows0, plan0.expert_counts, factors)
        got, back = comm.combineTokens(y, plan, wd, returnSlotRows=True)
        got0, back0 = comm.combineTokens(y0, plan0, wd, returnSlotRows=True)
        g = moe_ref.tokens(T, width, torch.float32, 77 + r).to("cuda")
        g_rows, g_w = comm.combineTokensBackward(g, plan, wd, back)
        g_rows0, g_w0 = comm.combineTokensBackward(g, plan0, wd, back0)
        torch.cuda.synchronize()
        row = dict(name=name, rows=same_bits(rows, rows0), slots=torch.equal(plan.slots, plan0.slots),
                   out=same_bits(got, got0), back=same_bits(back, back0), g_rows=same_bits(g_rows, g_rows0),
                   g_w=same_bits(g_w, g_w0), direct=same_bits(got.cpu(), moe_ref.direct(x, ids_m, w, E)),
                   untouched=torch.equal(idd.cpu(), ids) and same_bits(wd.cpu(), w),
                   counts=plan.expert_counts == plan0.expert_counts and plan.matrix == plan0.matrix,
                   cut=masked, used=used, exchanged=exchanged)
        neg = int((ids < 0).sum())
        if padded:
            row.update(kept=torch.equal(plan.kept, plan0.kept), valid=torch.equal(plan.valid, plan0.valid),
                       dropped=plan.dropped.tolist() == [masked, neg, 0] and plan.dropped.is_cuda
                       and plan0.dropped.tolist() == [0, neg + masked, 0])
        else:
            _, pos = comm.dispatchTokens(xd, idd, E, **kw)
            row.update(host=plan.expert_matrix == pos.expert_matrix and plan.demand_matrix == pos.demand_matrix
                       and plan.clipped == pos.clipped == masked and plan.matrix == pos.matrix and plan._clip is None
                       and plan.send_counts == pos.send_counts and plan.recv_counts == pos.recv_counts)
        out.append(row)
    return out


@pytest.mark.parametrize("padded", [True, False], ids=["padded", "capacity"])
@pytest.mark.parametrize("p", [2, 3])
def test_a_priority_dispatch_is_the_plain_call_on_the_masked_ids(p, padded):
    res = run_spawn(p, _api, args=(padded,))
    assert sorted(res) == list(range(p))
    for r, rows in res.items():
        for row in rows:
            what = (r, row["name"])
            for key, val in row.items():
                if key not in ("name", "cut", "used", "exchanged"):
                    assert val is True, (what, key)
            d = row["used"]
            assert d.get("moe.dispatch") == 1, (what, d)
            if padded:      # no count exchange and one copy plan, as the position call
                assert row["exchanged"] == 0 and d.get("moe.dispatch.padded") == 1, (what, d)
                assert sum(d.get(k, 0) for k in IPC) == 1, (what, d)
            else:           # the one count exchange of the position call
                assert row["exchanged"] == 1, what
    assert sum(row["cut"] for rows in res.values() for row in rows) > 0


# ---------------------------------------------------------------- captured
T, K, EL, WIDTH, S = 70, 2, 2, 8, 12


def _variant(v, r, p):
    """(x, ids, w) of rank r for replay v: uniform ids with drops; nearly everything to one expert (cut
    hard); few tokens' worth of distinct experts (nothing cut)."""
    E = EL * p
    g = torch.Generator().manual_seed(8000 + 10 * v + r)
    if v % 3 == 0:
        ids = torch.randint(-1, E, (T, K), generator=g)
    elif v % 3 == 1:
        ids = torch.where(torch.rand(T, K, generator=g) < 0.8, torch.full((T, K), (r + 1) % E),
                          torch.randint(0, E, (T, K), generator=g))
    else:
        ids = torch.full((T, K), -1)
        ids[:S // 2] = torch.randint(0, E, (S // 2, K), generator=g)
    return moe_ref.tokens(T, WIDTH, torch.float32, 8100 + 10 * v + r), ids, moe_ref.gate_weights(T, K, 8200 + 10 * v + r)


def _captured(comm):
    from mp4x.parallel import sparse
    r, p = comm.getRank(), comm.getSlaveNum()
    E = EL * p
    x = torch.zeros(T, WIDTH, device="cuda")
    ids = torch.zeros(T, K, dtype=torch.int64, device="cuda")
    w = torch.zeros(T, K, device="cuda")
    out = torch.zeros(T, WIDTH, device="cuda")
    state, factors = {}, _factors(r * EL, EL)

    def load(v):
        xv, iv, wv = _variant(v, r, p)
        x.copy_(xv)
        ids.copy_(iv)
        w.copy_(wv)

    def step():
        rows, plan = comm.dispatchTokens(x, ids, E, sourceCapacity=S, priority=w)
        out.copy_(comm.combineTokens(_padded_experts(rows, factors), plan, w))
        state["plan"] = plan

    load(0)
    gathers, gather = [], sparse._count_matrix
    sparse._count_matrix = lambda *a: gathers.append(1) or gather(*a)
    try:
        g = comm.device.capture(step)
    finally:
        sparse._count_matrix = gather
    plan = state["plan"]
    res = []
    for v in (1, 2, 3):
        load(v)
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        replayed = (out.clone(), plan.slots.clone(), plan.kept.clone(), plan.valid.clone(), plan.dropped.clone())
        xv, iv, wv = _variant(v, r, p)
        ids_m, masked = ref.mask_tensors(iv, wv, E, S)
        rows_e, plan_e = comm.dispatchTokens(x, ids, E, sourceCapacity=S, priority=w)             # eager, same inputs
        out_e = comm.combineTokens(_padded_experts(rows_e, factors), plan_e, w)
        rows_0, plan_0 = comm.dispatchTokens(x, ids_m.to("cuda"), E, sourceCapacity=S)             # plain, masked ids
        out_0 = comm.combineTokens(_padded_experts(rows_0, factors), plan_0, w)
        torch.cuda.synchronize()
        res.append(dict(out=same_bits(replayed[0], out_e) and same_bits(out_e, out_0),
                        slots=torch.equal(replayed[1], plan_e.slots) and torch.equal(replayed[1], plan_0.slots),
                        kept=torch.equal(replayed[2], plan_e.kept) and torch.equal(replayed[2], plan_0.kept),
                        valid=torch.equal(replayed[3], plan_e.valid) and torch.equal(replayed[3], plan_0.valid),
                        dropped=torch.equal(replayed[4], plan_e.dropped) and int(replayed[4][0]) == masked,
                        cut=masked))
    return res, len(gathers)


def test_a_captured_priority_step_replays_exactly_on_fresh_ids_and_priorities():
    res = run_spawn(2, _captured)
    assert sorted(res) == [0, 1]
    for r, (replays, gathers) in res.items():
        assert len(replays) == 3 and gathers == 0
        for v, row in enumerate(replays):
            for key in ("out", "slots", "kept", "valid", "dropped"):
                assert row[key], (r, v, key)
        cuts = [row["cut"] for row in replays]
        assert max(cuts) > 0 and min(cuts) == 0, (r, cuts)
