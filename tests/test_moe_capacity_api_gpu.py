"""dispatchTokens(capacity=) / combineTokens through the public API on the GPU (p processes sharing
cuda:0): the (case, capacity) table of tests/moe_capacity_ref.py, dispatch -> integer "experts" ->
combine, bit for bit against the first-come reference; the plan's capacity fields; one IPC all-to-all
per dispatch and per combine, one count exchange per dispatch and none per combine; the inputs
untouched."""
import pytest

torch = pytest.importorskip("torch")

import moe_capacity_ref as cap  # noqa: E402
import moe_ref  # noqa: E402
from moe_ref import same_bits  # noqa: E402
from spawn_ranks import run_spawn  # noqa: E402

pytestmark = pytest.mark.gpu

IPC = "all_to_all_v.ipc"


def _moved(stats, before):
    return {k: c - before.get(k, 0) for k, c in stats.items() if c != before.get(k, 0)}


def _api(comm):
    from mp4x.parallel import sparse
    r, p = comm.getRank(), comm.getSlaveNum()
    stats = comm.device.stats
    out = []
    for name, C in cap.TABLE:
        want = cap.end_to_end(name, p, C)[r]
        x, ids, w = want["x"].to("cuda"), want["ids"].to("cuda"), want["w"].to("cuda")
        gathers, gather = [], sparse._count_matrix
        sparse._count_matrix = lambda *a: gathers.append(1) or gather(*a)
        try:
            before = dict(stats)
            rows, plan = comm.dispatchTokens(x, ids, want["E"], capacity=C)
            torch.cuda.synchronize()
            d_used, d_gathers = _moved(stats, before), len(gathers)
            y = moe_ref.apply_experts(rows.cpu(), plan.expert_counts, r * (want["E"] // p)).to("cuda")
            before = dict(stats)
            got = comm.combineTokens(y, plan, w)
            torch.cuda.synchronize()
            c_used, c_gathers = _moved(stats, before), len(gathers) - d_gathers
            again = comm.combine_tokens(y, plan, w)
        finally:
            sparse._count_matrix = gather
        as_lists = lambda m: [list(row) for row in m]                                    # noqa: E731
        out.append(dict(name=(name, C), rows=same_bits(rows, want["rows"]),
                        counts=list(plan.expert_counts) == want["expert_counts"],
                        slots=torch.equal(plan.slots.cpu(), want["slots"]), out=same_bits(got, want["out"]),
                        again=same_bits(again, got), mat=as_lists(plan.matrix) == want["mat"],
                        emat=as_lists(plan.expert_matrix) == want["emat"],
                        demand=as_lists(plan.demand_matrix) == want["demand"],
                        clipped=plan.clipped == want["clipped"], capacity=plan.capacity == C,
                        kept=same_bits(x, want["x"]) and torch.equal(ids.cpu(), want["ids"]) and same_bits(w, want["w"]),
                        d_used=d_used, c_used=c_used, d_gathers=d_gathers, c_gathers=c_gathers))
    return out


@pytest.mark.parametrize("p", [2, 3])
def test_dispatch_experts_combine_under_a_capacity(p):
    res = run_spawn(p, _api)
    assert sorted(res) == list(range(p))
    for r, rows in res.items():
        assert [row["name"] for row in rows] == cap.TABLE
        for row in rows:
            what = (r, row["name"])
            for key in ("rows", "counts", "slots", "out", "again", "mat", "emat", "demand", "clipped", "capacity", "kept"):
                assert row[key], (what, key)
            assert row["d_used"].get("moe.dispatch") == 1 and row["d_used"].get(IPC) == 1, (what, row["d_used"])
            assert row["c_used"].get("moe.combine") == 1 and row["c_used"].get(IPC) == 1, (what, row["c_used"])
            assert "moe.combine" not in row["d_used"] and "moe.dispatch" not in row["c_used"], what
            assert (row["d_gathers"], row["c_gathers"]) == (1, 0), what
