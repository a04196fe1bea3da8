"""The GBDT kernels (csrc/kernels/gbdt.hip) against the CPU definitions of mp4x/parallel/gbdt.py, bit
for bit: every call runs twice into an output with sentinel guards on either side.  kTile is 4096 row
slots, so n = 5000 rows of one node cross two tiles."""
import pytest

torch = pytest.importorskip("torch")

import gbdt_cases as cases  # noqa: E402
from mp4x.parallel import gbdt  # noqa: E402

pytestmark = pytest.mark.gpu

NS, FS, BS, KS = (1, 111, 600, 5000), (1, 5, 16, 37), (2, 16, 255, 256), (1, 3, 64)
HIST = [dict(n=n, F=F, B=BS[(i + j) % 4], k=KS[(i + 2 * j) % 3]) for i, n in enumerate(NS) for j, F in enumerate(FS)] + \
       [dict(n=5000, F=37, B=256, k=1), dict(n=5000, F=16, B=256, k=64), dict(n=600, F=37, B=255, k=3),
        dict(n=5000, F=1, B=2, k=1), dict(n=5000, F=5, B=256, k=1), dict(n=111, F=37, B=256, k=64),
        dict(n=5000, F=37, B=16, k=3, one_node=True), dict(n=5000, F=37, B=256, k=1, one_bin=True),
        dict(n=5000, F=1, B=256, k=1, one_bin=True), dict(n=5000, F=5, B=16, k=3, bad_rows=True),
        dict(n=600, F=37, B=16, k=3, high_bins=True)] + \
       [dict(n=5000, F=5, B=16, k=4, seg=s) for s in cases.HOSTILE.values()]


def _twice(call, shape, dtype):
    outs = []
    for _ in range(2):
        buf, out = cases.guarded(shape, dtype, "cuda")
        call(out)
        torch.cuda.synchronize()
        assert cases.guards_intact(buf)
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1])
    return outs[0]


@pytest.mark.parametrize("case", HIST, ids=lambda c: "-".join(f"{k}{v if k != 'seg' else ''}" for k, v in c.items()))
def test_histogram_kernel_equals_the_definition(case):
    from mp4x.ops import device_ops
    bins, gh, rows, seg = cases.hist_case(**case)
    want = gbdt.gbdt_hist_torch(bins, gh, rows, seg, case["B"])
    dev = [t.cuda() for t in (bins, gh, rows, seg)]
    got = _twice(lambda out: device_ops.gbdt_histogram(*dev, case["B"], out=out), want.shape, torch.int64)
    assert torch.equal(got, want)


def test_histogram_of_no_row_slots_is_zero():
    from mp4x.ops import device_ops
    bins, gh, _, _ = cases.hist_case(111, 5, 16, 3)
    rows, seg = torch.zeros(0, dtype=torch.int32, device="cuda"), torch.tensor([0, 5, 9, 9], device="cuda")
    got = _twice(lambda out: device_ops.gbdt_histogram(bins.cuda(), gh.cuda(), rows, seg, 16, out=out), (3, 5, 16, 2),
                 torch.int64)
    assert not got.any()


def test_sums_past_two_to_the_53_are_exact():
    from mp4x.ops import device_ops
    n = 2 ** 23
    bins = torch.ones(n, 1, dtype=torch.uint8, device="cuda")
    gh = torch.tensor([cases.QMAX, -cases.QMAX], dtype=torch.int32, device="cuda").repeat(n, 1)
    rows, seg = torch.arange(n, dtype=torch.int32, device="cuda"), torch.tensor([0, n], device="cuda")
    got = _twice(lambda out: device_ops.gbdt_histogram(bins, gh, rows, seg, 2, out=out), (1, 1, 2, 2), torch.int64)
    assert got.tolist() == [[[[0, 0], [n * cases.QMAX, -n * cases.QMAX]]]] and n * cases.QMAX > 2 ** 53


def test_quantize_kernel_equals_the_definition():
    from mp4x.ops import device_ops
    (gv, sg), (hv, sh) = cases.QUANT_G, cases.QUANT_H
    g, h = torch.tensor(gv, dtype=torch.float32), torch.tensor(hv, dtype=torch.float32)    # 17 rows: an odd tail
    want = gbdt.gbdt_quantize_torch(g, h, sg, sh)
    got = _twice(lambda out: device_ops.gbdt_quantize(g.cuda(), h.cuda(), sg, sh, out=out), (len(gv), 2), torch.int32)
    assert torch.equal(got, want)


SPLITS = [(n, *cases.SPLIT[n][:4]) for n in sorted(cases.SPLIT)] + \
         [(f"random-F{F}-B{B}", cases.random_hist(3, F, B, F + B), 35, 29, 1.0) for F in (1, 37) for B in (2, 256)]


@pytest.mark.parametrize("name,hist,sg,sh,lam", SPLITS, ids=[s[0] for s in SPLITS])
def test_split_kernel_equals_the_definition(name, hist, sg, sh, lam):
    from mp4x.ops import device_ops
    want = gbdt.gbdt_split_torch(hist, sg, sh, lam)
    k, runs = hist.shape[0], []
    for _ in range(2):
        pairs = [cases.guarded((k,), t.dtype, "cuda", guard=2) for t in want]
        device_ops.gbdt_best_split(hist.cuda(), sg, sh, lam, out=device_ops.GbdtSplit(*(v for _, v in pairs)))
        torch.cuda.synchronize()
        assert all(cases.guards_intact(buf, guard=2) for buf, _ in pairs)
        runs.append([v.cpu() for _, v in pairs])
    for a, b, w, field in zip(runs[0], runs[1], want, want._fields):
        if field == "gain":
            a, b, w = a.view(torch.int64), b.view(torch.int64), w.view(torch.int64)        # equal as bits
        assert torch.equal(a, b) and torch.equal(a, w), (field, a, w)
