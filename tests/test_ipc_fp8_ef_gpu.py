"""The fp8 reduce-scatter with error feedback (IpcAllreduce.reduce_scatter_fp8(residual=...)), p
processes sharing ONE GPU, a 64 KiB staging buffer so the larger cases run in several pieces.

With Q_ef = fp8_ef_ref.ref_quant_ef, R = ref_dequant_reduce, S = ref_store: after step t, rank r's
segment is the slice of S(R([Q_ef(x_0[base:end], r_0), ..., Q_ef(x_{p-1}[base:end], r_{p-1})])), its
residual is Q_ef's for rank r, and everything else keeps its bits — over three steps chained on the
same residual tensors, bit for bit."""
import pytest

torch = pytest.importorskip("torch")

from fp8_ef_ref import ref_quant_ef  # noqa: E402
from fp8_ref import ref_dequant_reduce, ref_store  # noqa: E402
from fp8_rsag_ref import CASES, bounds, expect_reduce_scatter, same_bits  # noqa: E402
from spawn_ranks import run_spawn  # noqa: E402

pytestmark = pytest.mark.gpu

STEPS = 3


def _inputs(n, dtype, p, step):
    """Every rank's input of one step, built on the CPU, the same in every process."""
    return [torch.randn(n, generator=torch.Generator().manual_seed(900 + 10 * step + j)).to(dtype) for j in range(p)]


def _expect(xs, resids, r, frm, counts):
    """(rank r's tensor after the call, every rank's new residual, ambiguous)."""
    froms, tos = bounds(frm, counts)
    base, end = froms[0], tos[-1]
    qs, ss, new, amb = [], [], [], 0
    for x, res in zip(xs, resids):
        q, s, nr, a = ref_quant_ef(x[base:end], res)
        qs.append(q)
        ss.append(s)
        new.append(nr)
        amb += a
    acc, a = ref_dequant_reduce(qs, ss)
    full = ref_store(acc, xs[0].dtype)
    out = xs[r].clone()
    out[froms[r]:tos[r]] = full[froms[r] - base:tos[r] - base]
    return out, new, amb + a


def _dev(t, offset):
    """A device copy of ``t``, 4 bytes off the 16-byte grid when ``offset``."""
    n = t.numel()
    if offset:
        assert t.element_size() == 4
        buf = torch.empty(n + 4, dtype=t.dtype, device="cuda")
        y = buf[1:1 + n]
        assert y.data_ptr() % 16 == 4
    else:
        y = torch.empty(n, dtype=t.dtype, device="cuda")
        assert y.data_ptr() % 16 == 0
    y.copy_(t)
    return y


def _worker(comm):
    from mp4x.parallel.ipc import IpcAllreduce
    r, p = comm.getRank(), comm.getSlaveNum()
    ipc = IpcAllreduce(comm, nbytes=64 << 10)
    out = []
    # every case; case A again with rank 1's tensor, then rank 1's residual, 4 bytes off the grid
    runs = [(name, None) for name in CASES] + [("A", "tensor"), ("A", "residual")]
    for name, odd in runs:
        dtype_name, n, frm, counts = CASES[name]
        counts = counts[p]
        dtype = getattr(torch, dtype_name)
        froms, tos = bounds(frm, counts)
        nres = tos[-1] - froms[0]
        ref_res = [torch.zeros(nres) for _ in range(p)]
        res = _dev(ref_res[r], odd == "residual" and r == 1)
        for step in range(STEPS):
            xs = _inputs(n, dtype, p, step)
            want, ref_res, amb = _expect(xs, ref_res, r, frm, counts)
            y = _dev(xs[r], odd == "tensor" and r == 1)
            ok = ipc.reduce_scatter_fp8(y, froms, tos, residual=res)
            torch.cuda.synchronize()
            got = y.cpu()
            keep = torch.ones(n, dtype=torch.bool)
            keep[froms[r]:tos[r]] = False
            out.append(dict(case=name, odd=odd, step=step, ok=bool(ok), amb=amb, ew=ipc.error_word(),
                            equal=same_bits(got, want), untouched=same_bits(got[keep], xs[r][keep]),
                            resid=same_bits(res, ref_res[r]), ndiff=int((got != want).sum()),
                            nres=int((res.cpu() != ref_res[r]).sum())))
            if name == "A" and odd is None and step == 0:
                # a call without a residual between two with one: today's contract, residual untouched
                xs0 = _inputs(n, dtype, p, 7)
                want0, amb0 = expect_reduce_scatter(xs0, r, frm, counts)
                y0 = _dev(xs0[r], False)
                ok0 = ipc.reduce_scatter_fp8(y0, froms, tos)
                torch.cuda.synchronize()
                out.append(dict(case=name, odd="plain call", step=step, ok=bool(ok0), amb=amb0, ew=ipc.error_word(),
                                equal=same_bits(y0, want0), untouched=True, resid=same_bits(res, ref_res[r]),
                                ndiff=int((y0.cpu() != want0).sum()), nres=0))
    # refusals come before any piece: the epoch stays in step and the next call still runs
    from mp4x.exceptions import Mp4jException
    dtype_name, n, frm, counts = CASES["A"]
    froms, tos = bounds(frm, counts[p])
    y = torch.zeros(n, device="cuda")
    refused = 0
    for bad in (torch.zeros(n - 4, device="cuda"), torch.zeros(n, device="cuda", dtype=torch.float16), torch.zeros(n)):
        try:
            ipc.reduce_scatter_fp8(y, froms, tos, residual=bad)
        except Mp4jException:
            refused += 1
    # a range that does not qualify: False, the residual untouched
    res = torch.full((n - 2,), 0.25, device="cuda")
    not_run = ipc.reduce_scatter_fp8(y, [0] + [258] * (p - 1), [258] * (p - 1) + [n - 2], residual=res)
    y.fill_(float(r + 1))
    again = ipc.reduce_scatter_fp8(y, froms, tos, residual=torch.zeros(n, device="cuda"))
    torch.cuda.synchronize()
    tail = dict(refused=refused, not_run=bool(not_run), res_kept=bool((res == 0.25).all()), again=bool(again),
                ew=ipc.error_word(), mine=y[froms[r]:tos[r]].cpu().tolist())
    comm.barrier()
    ipc.close()
    return out, tail


@pytest.mark.parametrize("p", [2, 3])
def test_fp8_reduce_scatter_with_error_feedback_bit_for_bit(p):
    res = run_spawn(p, _worker)
    assert sorted(res) == list(range(p))
    nrun = len(res[0][0])
    assert nrun == STEPS * (len(CASES) + 2) + 1
    for i in range(nrun):
        for r in range(p):
            row = res[r][0][i]
            what = (row["case"], row["odd"], row["step"], r)
            assert row["amb"] == 0, what          # a condition on the inputs: change a seed, never the comparison
            assert row["ok"], what
            assert row["ew"] == 0, what
            assert row["equal"], (what, row["ndiff"])
            assert row["untouched"], what
            assert row["resid"], (what, row["nres"])
    # (the offset runs of case A are held to the reference of the aligned run: the same bits)
    want = float(sum(range(1, p + 1)))
    for r in range(p):
        tail = res[r][1]
        assert tail["refused"] == 3 and not tail["not_run"] and tail["res_kept"] and tail["again"], tail
        assert tail["ew"] == 0
        # constants k + 1 encode as the code 448 under the scale (k + 1) / 448: exact to an ulp each
        assert all(abs(v - want) <= want * 2.0 ** -22 for v in tail["mine"]), tail["mine"][:4]
