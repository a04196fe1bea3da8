"""dispatchTokens / combineTokens through the public API on the GPU (p processes sharing cuda:0):
dispatch -> integer "experts" -> combine for the four cases of tests/moe_ref.py, bit for bit; one
IPC all-to-all per dispatch and per combine, one count exchange per dispatch and none per combine;
and the fp8 operand, handed to the all-to-all unchanged."""
import pytest

torch = pytest.importorskip("torch")

import moe_ref  # noqa: E402
from moe_ref import CASES, same_bits  # noqa: E402
from spawn_ranks import run_spawn  # noqa: E402

pytestmark = pytest.mark.gpu

FP8, IPC = "all_to_all_v.fp8.ipc", "all_to_all_v.ipc"


def _moved(stats, before):
    return {k: c - before.get(k, 0) for k, c in stats.items() if c != before.get(k, 0)}


def _api(comm):
    from mp4x.parallel import sparse
    r, p = comm.getRank(), comm.getSlaveNum()
    stats = comm.device.stats
    out = []
    for name in sorted(CASES):
        want = moe_ref.end_to_end(name, p)[r]
        x, ids, w = want["x"].to("cuda"), want["ids"].to("cuda"), want["w"].to("cuda")
        gathers, gather = [], sparse._count_matrix
        sparse._count_matrix = lambda *a: gathers.append(1) or gather(*a)
        try:
            before = dict(stats)
            rows, plan = comm.dispatchTokens(x, ids, want["E"])
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
        out.append(dict(name=name, rows=same_bits(rows, want["rows"]),
                        counts=list(plan.expert_counts) == want["expert_counts"],
                        slots=torch.equal(plan.slots.cpu(), want["slots"]), out=same_bits(got, want["out"]),
                        again=same_bits(again, got), kept=same_bits(x, want["x"]),
                        d_used=d_used, c_used=c_used, d_gathers=d_gathers, c_gathers=c_gathers))
    return out


@pytest.mark.parametrize("p", [2, 3])
def test_dispatch_experts_combine(p):
    res = run_spawn(p, _api)
    assert sorted(res) == list(range(p))
    for r, rows in res.items():
        assert len(rows) == 4
        for row in rows:
            what = (r, row["name"])
            for key in ("rows", "counts", "slots", "out", "again", "kept"):
                assert row[key], (what, key)
            assert row["d_used"].get("moe.dispatch") == 1 and row["d_used"].get(IPC) == 1, (what, row["d_used"])
            assert row["c_used"].get("moe.combine") == 1 and row["c_used"].get(IPC) == 1, (what, row["c_used"])
            assert "moe.combine" not in row["d_used"] and "moe.dispatch" not in row["c_used"], what
            assert (row["d_gathers"], row["c_gathers"]) == (1, 0), what


def _fp8(comm):
    from mp4x import Mp4jException, Operands
    r, p = comm.getRank(), comm.getSlaveNum()
    stats = comm.device.stats
    per_rank, routes = moe_ref.check_case_properties("D8", p)
    x, ids, w, E = per_rank[r]
    K = ids.shape[1]
    operand = Operands.BF16_OPERAND(codec="fp8")
    before = dict(stats)
    rows, plan = comm.dispatchTokens(x.to("cuda"), ids.to("cuda"), E, operand=operand)
    torch.cuda.synchronize()
    used = _moved(stats, before)
    # the same transport call on the reference-routed send buffer, then the reference regroup
    sends = [moe_ref.ref_send(xx, rt[2], K) for (xx, _, _, _), rt in zip(per_rank, routes)]
    mat = moe_ref.ref_exchange(sends, routes, E)[r][3]
    recv, _ = comm.alltoallArray(sends[r].to("cuda"), mat[r], operand=operand)
    torch.cuda.synchronize()
    el = E // p
    cnt = [rt[0][:E].tolist() for rt in routes]
    seg, off = {}, 0
    for i in range(p):
        for e in range(el):
            c = cnt[i][r * el + e]
            seg[(i, e)] = recv[off:off + c]
            off += c
    want = torch.cat([seg[(i, e)] for e in range(el) for i in range(p)])
    exact = moe_ref.ref_exchange(sends, routes, E)[r][0]
    # a capture is refused before anything moves (the capture state is stubbed: nothing is captured)
    from mp4x.ops import native
    refused, real = False, native.capturing_now
    native.capturing_now = lambda: True
    try:
        comm.dispatchTokens(x.to("cuda"), ids.to("cuda"), E)
    except Mp4jException as e:
        refused = "capture" in str(e)
    finally:
        native.capturing_now = real
    try:
        native.capturing_now = lambda: True
        comm.combineTokens(rows, plan)
        refused = False
    except Mp4jException as e:
        refused = refused and "capture" in str(e)
    finally:
        native.capturing_now = real
    return dict(equal=same_bits(rows, want), lossy=not same_bits(rows, exact), fp8=used.get(FP8, 0),
                ipc=used.get(IPC, 0), rows=rows.shape[0], refused=refused)


def test_fp8_operand_reaches_the_all_to_all():
    res = run_spawn(2, _fp8)
    assert sorted(res) == [0, 1]
    for r, row in res.items():
        assert (row["fp8"], row["ipc"]) == (1, 0), (r, row)
        assert row["equal"], r
        assert row["refused"], r
        if row["rows"]:
            assert row["lossy"], r                       # e4m3 was on the wire
