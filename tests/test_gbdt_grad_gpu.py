"""The GBDT loss kernels (csrc/kernels/gbdt_grad.hip) against the CPU definitions of mp4x/parallel/gbdt.py, bit for
bit (a NaN of ``top`` equal to any NaN), twice into outputs with sentinel guards on either side: n around the pair
store's tail and the 256-lane and 1024-row block edges, the hostile margins, per-class shifts and shifts at and past
+-200; one capture and replay; one small softmax model against the CPU."""
import pytest

torch = pytest.importorskip("torch")

import gbdt_cases as cases  # noqa: E402
import gbdt_grad_cases as gcases  # noqa: E402
from mp4x.parallel import gbdt  # noqa: E402
from spawn_ranks import run_spawn  # noqa: E402

pytestmark = pytest.mark.gpu

NS = (0, 1, 2, 3, 255, 256, 257, 2 * 256 + 1, 1024 + 3)
FORMS = [("squared", 1), ("logistic", 1), ("softmax", 2), ("softmax", 3), ("softmax", 7)]


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("loss,C", FORMS)
def test_kernels_equal_the_definitions(loss, C, n):
    from mp4x.ops import device_ops
    pred, y = gcases.margins(loss, n, C, seed=n)
    dev = (pred.cuda(), y.cuda())
    want_top = gbdt.gbdt_grad_absmax_torch(pred, y, loss)
    tops = []
    for wide in (False, True):
        sg, sh = gcases.shifts(C, wide)
        want = gbdt.gbdt_grad_quantize_torch(pred, y, loss, sg, sh)
        tbuf, top = cases.guarded((C, 2), torch.float32, "cuda")
        gbuf, gh = cases.guarded((C, n, 2), torch.int32, "cuda")
        assert gbdt.gbdt_grad_absmax_torch(*dev, loss, out=top) is top
        assert device_ops.gbdt_grad_quantize(*dev, loss, sg.cuda(), sh.cuda(), out=gh) is gh
        torch.cuda.synchronize()
        assert cases.guards_intact(tbuf) and cases.guards_intact(gbuf)
        assert gcases.same_floats(top.cpu(), want_top), (top.cpu(), want_top)
        assert torch.equal(gh.cpu(), want)
        tops.append(top.cpu().view(torch.int32))
    assert torch.equal(tops[0], tops[1])                       # run twice: the same bits, a NaN's too


def _captured(comm):
    from mp4x.ops import device_ops
    pred, y = (t.cuda() for t in gcases.margins("softmax", 700, 3, finite=True))
    sg, sh = (t.cuda() for t in gcases.shifts(3))
    top = torch.zeros(3, 2, device="cuda")
    gh = torch.zeros(3, 700, 2, dtype=torch.int32, device="cuda")

    def step():
        device_ops.gbdt_grad_absmax(pred, y, "softmax", out=top)
        device_ops.gbdt_grad_quantize(pred, y, "softmax", sg, sh, out=gh)

    graph = comm.device.capture(step)
    same = []
    for v in (1, 2, 3):
        pred.copy_(gcases.margins("softmax", 700, 3, seed=v, finite=True)[0])
        top.fill_(9.0)                                         # a replay zeroes top itself
        graph.replay()
        torch.cuda.synchronize()
        same.append(torch.equal(top.cpu(), gbdt.gbdt_grad_absmax_torch(pred.cpu(), y.cpu(), "softmax")) and
                    torch.equal(gh.cpu(), gbdt.gbdt_grad_quantize_torch(pred.cpu(), y.cpu(), "softmax", sg.cpu(), sh.cpu())))
    return same


def test_a_captured_round_replays_exactly_and_the_gpu_grows_the_cpus_softmax_trees():
    assert run_spawn(1, _captured)[0] == [True] * 3
    bins, cls = gcases.class_data()
    settings = dict(trees=2, depth=3, loss="softmax", classes=3, level="partition", update="walk")
    want = gbdt.train_gbdt_quantized(None, bins, cls, 16, **settings)
    got = gbdt.train_gbdt_quantized(None, bins.cuda(), cls.cuda(), 16, **settings)
    assert len(want) == 6 and len(want[0].value) > 1
    assert [cases.tree_tuple(t) for t in got] == [cases.tree_tuple(t) for t in want]
    margins = gbdt.predict_gbdt(got, bins.cuda(), classes=3)
    assert torch.equal(margins.cpu(), gbdt.predict_gbdt(want, bins, classes=3))
