"""The group-limited router gate on the CPU (mp4x/models/moe.py: ``route_topk_grouped``, its torch form
and its closed-form backward) against the float64 definition of tests/moe_gate_group_ref.py: scores,
weights, lse, prob_sum and the gradient inside the derived bounds (DESIGN "K13"), the selection by
the tolerance-aware check everywhere and exactly on the separated fixtures, which are asserted to be
separated; without a bias and with one group the ids are the plain gate's definition's
(tests/moe_gate_ref.py) and the softmax score gives ``route_topk``'s bits."""
import pytest

torch = pytest.importorskip("torch")

import moe_gate_group_ref as ref  # noqa: E402
import moe_gate_ref  # noqa: E402
from moe_ref import same_bits  # noqa: E402
from mp4x.models.moe import (gate_group_backward_torch, gate_group_forward_torch, route_topk,  # noqa: E402
                             route_topk_grouped)

T = 65
SHAPES = [(8, 4, 2, 2), (6, 3, 2, 4), (60, 5, 3, 6), (64, 8, 4, 8), (64, 1, 1, 8), (256, 8, 4, 8), (260, 4, 1, 16),
          (2048, 32, 8, 16)]


def _forward_checks(res, want, what, exact=False):
    ids = res.ids.to(torch.int64)
    assert want.selection_ok(res.group_ids, ids) is None, (what, want.selection_ok(res.group_ids, ids))
    if exact:
        assert torch.equal(res.group_ids.to(torch.int64), want.group_ids), (what, "group_ids")
        assert torch.equal(ids, want.ids), (what, "ids")
    rows = [("weights", res.weights, want.weights(ids)[0], want.weights_bound(ids))]
    if want.score == "softmax":
        rows.append(("lse", res.lse, want.lse, want.lse_bound()))
    else:
        assert res.lse is None
    if res.prob_sum is not None:
        rows.append(("prob_sum", res.prob_sum, want.prob_sum, want.prob_sum_bound()))
        assert torch.equal(res.counts, torch.bincount(ids.reshape(-1), minlength=want.E)), (what, "counts")
    for name, got, w64, bound in rows:
        ok, ratio = ref.inside(got, w64, bound)
        print(what, name, "worst / bound = %.3f" % ratio)
        assert ok, (what, name, ratio)


@pytest.mark.parametrize("score", ["sigmoid", "softmax"])
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_and_backward_inside_the_bounds(shape, score):
    E, Gr, Kg, K = shape
    for n, (with_bias, renormalize) in enumerate(((False, False), (True, True), (True, False), (False, True))):
        R, scale = (4, 32)[n % 2], (1.0, 2.5)[n % 2]
        logits, bias, want = ref.uniform_case(T, E, Gr, Kg, K, score, with_bias, renormalize, scale, R, 100 + E + n, "float32")
        what = (shape, score, with_bias, renormalize)
        # the selection scores themselves: c of the torch form inside delta
        lg = logits.clone().requires_grad_(True)
        res = route_topk_grouped(lg, K, score=score, bias=bias, n_group=Gr, topk_group=Kg, renormalize=renormalize,
                                 scale=scale, stats=True)
        _forward_checks(res, want, what)
        assert res.weights.requires_grad and res.prob_sum.requires_grad
        assert not res.ids.requires_grad and not res.counts.requires_grad and not res.group_ids.requires_grad
        ids = res.ids.to(torch.int64)
        grads = ref.gradients(T, E, K, 200 + E + n)
        if score == "sigmoid":
            grads = (grads[0], None, grads[2])
        g64, bound = want.backward(ids, *grads)
        loss = (res.weights * grads[0]).sum() + (res.prob_sum * grads[2]).sum()
        if score == "softmax":
            loss = loss + (res.lse * grads[1]).sum()
        loss.backward()
        ok, ratio = ref.inside(lg.grad, g64, bound)
        print(what, "g_logits worst / bound = %.3f" % ratio)
        assert ok, (what, ratio)


@pytest.mark.parametrize("shape", [(64, 8, 4, 8), (256, 8, 4, 8), (2048, 32, 8, 16)])
def test_the_selection_scores_are_inside_delta_and_a_permuted_choice_is_rejected(shape):
    E, Gr, Kg, K = shape
    logits, bias, want = ref.uniform_case(T, E, Gr, Kg, K, "sigmoid", True, True, 2.5, 4, 100 + E + 1, "float32")
    c32 = 1.0 / (1.0 + torch.exp(-logits)) + bias
    ok, ratio = ref.inside(c32, want.c, want.delta)
    print(shape, "c worst / bound = %.3f" % ratio)
    assert ok, ratio
    gs32 = ref.group_scores(c32, Gr)
    ok, ratio = ref.inside(gs32, want.gs, want.delta_g)
    print(shape, "group score worst / bound = %.3f" % ratio)
    assert ok, ratio
    res = route_topk_grouped(logits, K, bias=bias, n_group=Gr, topk_group=Kg, renormalize=True, scale=2.5)
    assert want.selection_ok(res.group_ids, res.ids) is None
    assert want.selection_ok(res.group_ids, res.ids.flip(1)) is not None               # ascending
    assert want.selection_ok(res.group_ids, (res.ids + E // Gr) % E) is not None        # another group's columns
    other = (res.group_ids + 1) % Gr
    assert want.selection_ok(other, res.ids) is not None
    twice = res.ids.clone()
    twice[:, 1] = twice[:, 0]
    assert want.selection_ok(res.group_ids, twice) is not None


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("i", range(len(ref.SEPARATED)))
def test_the_separated_fixtures_are_separated_and_their_ids_exact(i, dtype):
    kind, E, Gr, Kg, K, score, _ = ref.SEPARATED[i]
    logits, bias, want = ref.separated_case(i, T, dtype)
    assert ref.separated(want) is None, (ref.SEPARATED[i], ref.separated(want))
    for ids_dtype in (torch.int64, torch.int32):
        res = route_topk_grouped(logits, K, score=score, bias=bias, n_group=Gr, topk_group=Kg, renormalize=True,
                                 scale=2.5, ids_dtype=ids_dtype, stats=True)
        assert res.ids.dtype == ids_dtype and res.group_ids.dtype == torch.int32
        _forward_checks(res, want, (ref.SEPARATED[i], dtype), exact=True)
    # the backward with masked (-inf) columns: their gradient is exactly zero
    grads = ref.gradients(T, E, K, 800 + i)
    grads = (grads[0], None, grads[2]) if score == "sigmoid" else grads
    g64, bound = want.backward(want.ids, *grads)
    got = gate_group_backward_torch(logits, res.lse, want.ids, score, True, 2.5, *grads)
    ok, ratio = ref.inside(got, g64, bound)
    assert ok, (ref.SEPARATED[i], dtype, ratio)
    assert not bool(got[logits == float("-inf")].to(torch.float32).abs().max() > 0)


def test_separation_is_a_condition_that_can_fail():
    # symmetric integer logits: sigma(2) + sigma(-2) and sigma(0) + sigma(0) tie in exact arithmetic only
    lg = torch.tensor([[2.0, -2.0, 0.0, 0.0]])
    assert ref.separated(ref.Reference(lg, 1, "sigmoid", None, 2, 1, False, 1.0)) == "two groups too close"
    # a two-level bias with groups: (a + b1) + c against a + (c + b1)
    lg = torch.tensor([[1.0, 2.0, 2.0, 1.0]])
    bias = torch.tensor([0.3, 0.0, 0.3, 0.0])
    assert ref.separated(ref.Reference(lg, 1, "sigmoid", bias, 2, 1, False, 1.0)) == "two groups too close"
    lg = torch.tensor([[1.0, 1.0 + 2.0 ** -12, 3.0, 4.0]])
    assert ref.separated(ref.Reference(lg, 1, "sigmoid", None, 1, 1, False, 1.0)) == "two columns too close"


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
def test_no_bias_and_one_group_give_the_ids_of_the_plain_gate(dtype):
    dt = getattr(torch, dtype)
    for E in (1, 2, 5, 64, 257):
        for K in sorted({min(k, E) for k in (1, 2, 8, 16)}):
            # the float64 definition of the plain gate (tests/moe_gate_ref.py), not the code under test
            logits, want = moe_gate_ref.cached_reference("ties", T, E, K, True, 0, 500 + E, dtype)
            for score in ("softmax", "sigmoid"):
                res = route_topk_grouped(logits, K, score=score, renormalize=True)
                assert torch.equal(res.ids, moe_gate_ref.order_ids(logits, K)), (E, K, score)
                assert bool((res.group_ids == 0).all()) and res.group_ids.shape == (T, 1)
            # the softmax score with nothing else is the plain gate: inside the plain gate's own bounds ...
            lg = logits.clone().requires_grad_(True)
            res = route_topk_grouped(lg, K, score="softmax", renormalize=True, stats=True)
            assert moe_gate_ref.inside(res.weights, want.w, want.weights_bound())[0], (E, K, "weights")
            assert moe_gate_ref.inside(res.lse, want.lse, want.lse_bound())[0], (E, K, "lse")
            # ... and route_topk bit for bit, forward and backward of the same scalar
            lp = logits.clone().requires_grad_(True)
            plain = route_topk(lp, K, True, stats=True)
            assert same_bits(res.weights, plain.weights) and same_bits(res.lse, plain.lse), (E, K)
            assert same_bits(res.prob_sum, plain.prob_sum), (E, K, "prob_sum")
            assert torch.equal(res.ids, plain.ids) and torch.equal(res.counts, plain.counts), (E, K)
            grads = moe_gate_ref.gradients(T, E, K, 600 + E)
            for r, leaf in ((res, lg), (plain, lp)):
                ((r.weights * grads[0]).sum() + (r.lse * grads[1]).sum() + (r.prob_sum * grads[2]).sum()).backward()
                assert leaf.grad.dtype == dt
            assert same_bits(lg.grad, lp.grad), (E, K, "logits.grad")
    nan, inf = float("nan"), float("inf")
    for E, K, Gr, Kg in ((5, 5, 1, 1), (64, 8, 1, 1), (257, 16, 1, 1), (64, 8, 8, 4), (2048, 16, 32, 8)):
        lg = moe_gate_ref.uniform_logits(9, E, 4, 77)
        lg[0] = nan
        lg[1] = inf
        lg[2] = -inf
        lg[3, ::2] = nan
        lg[4, 1::3] = inf
        lg[6, :E // 2] = -nan
        for bias in (None, ref.random_bias(E, 5)):
            res = route_topk_grouped(lg.to(dt), K, bias=bias, n_group=Gr, topk_group=Kg, renormalize=True)
            ids, gids = res.ids, res.group_ids.to(torch.int64)
            assert bool(((ids >= 0) & (ids < E)).all()) and all(len(set(r)) == K for r in ids.tolist())
            assert bool(((gids >= 0) & (gids < Gr)).all()) and all(len(set(r)) == Kg for r in gids.tolist())
            assert bool(((ids // (E // Gr)).unsqueeze(2) == gids.unsqueeze(1)).any(dim=-1).all())
            if Gr == 1 and bias is None:
                # every row, the NaN and infinite ones included, as a stable descending sort of the
                # float32 logits orders it; the ordinary rows as the definition
                order = torch.sort(lg.to(dt).to(torch.float32), dim=-1, descending=True, stable=True).indices[:, :K]
                assert torch.equal(ids, order)
                assert torch.equal(ids[7:], moe_gate_ref.order_ids(lg.to(dt)[7:], K))


@pytest.mark.parametrize("score", ["sigmoid", "softmax"])
@pytest.mark.parametrize("renormalize", [False, True])
@pytest.mark.parametrize("which", ref.GRAD_SETS)
def test_backward_with_every_combination_of_absent_gradients(which, renormalize, score):
    if score == "sigmoid":
        which = (which[0], 0, which[2])                # the sigmoid score has no lse: its gradient is always absent
    for (E, Gr, Kg, K), dtype in (((6, 3, 2, 4), "float32"), ((64, 8, 4, 8), "float32"), ((260, 4, 1, 16), "bfloat16"),
                                  ((64, 8, 4, 2), "float16")):
        logits, bias, want = ref.uniform_case(T, E, Gr, Kg, K, score, True, renormalize, 2.5, 4, 300 + E, dtype)
        grads = ref.pick(ref.gradients(T, E, K, 400 + E), which)
        w, ids, lse, _, _, gids = gate_group_forward_torch(logits, K, score, bias, Gr, Kg, renormalize, 2.5, torch.int64, False)
        assert want.selection_ok(gids, ids) is None
        g64, bound = want.backward(ids, *grads)
        got = gate_group_backward_torch(logits, lse, ids, score, renormalize, 2.5, *grads)
        assert got.dtype == logits.dtype
        ok, ratio = ref.inside(got, g64, bound)
        assert ok, (E, K, dtype, which, ratio)
        lg = logits.clone().requires_grad_(True)
        res = route_topk_grouped(lg, K, score=score, bias=bias, n_group=Gr, topk_group=Kg, renormalize=renormalize,
                                 scale=2.5, stats=True)
        terms = [(o * g).sum() for o, g in zip((res.weights, res.lse, res.prob_sum), grads) if g is not None]
        if terms:
            sum(terms).backward()
            ok, ratio = ref.inside(lg.grad, g64, bound)
            assert ok, (E, K, dtype, which, "autograd", ratio)
        else:
            assert not bool(got.to(torch.float32).abs().max() > 0)


def test_empty_and_refusals():
    for stats in (False, True):
        res = route_topk_grouped(torch.empty(0, 8, requires_grad=True), 3, n_group=4, topk_group=2, stats=stats)
        assert res.weights.shape == (0, 3) and res.ids.shape == (0, 3) and res.group_ids.shape == (0, 2) and res.lse is None
        if stats:
            assert res.prob_sum.tolist() == [0.0] * 8 and res.counts.tolist() == [0] * 8
        else:
            assert res.prob_sum is None and res.counts is None
    lg = torch.zeros(3, 8)
    for kw in (dict(top_k=0), dict(top_k=9), dict(top_k=True), dict(top_k=2.0), dict(score="tanh"), dict(n_group=3),
               dict(n_group=0), dict(n_group=4, topk_group=5), dict(n_group=4, topk_group=0), dict(n_group=4, topk_group=1, top_k=3),
               dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")), dict(scale=float("nan")),
               dict(bias=torch.zeros(7)), dict(bias=torch.zeros(8, dtype=torch.float64)), dict(bias=[0.0] * 8),
               dict(ids_dtype=torch.int16)):
        kw = dict(dict(top_k=2), **kw)
        with pytest.raises(ValueError, match="route_topk_grouped"):
            route_topk_grouped(lg, kw.pop("top_k"), **kw)
    with pytest.raises(ValueError, match="route_topk_grouped"):
        route_topk_grouped(torch.zeros(8), 1)
    # outside the kernel's range the same definition runs in torch: 64 groups
    logits, bias, want = ref.uniform_case(5, 128, 64, 9, 17, "sigmoid", True, True, 1.5, 4, 9, "float32")
    res = route_topk_grouped(logits, 17, bias=bias, n_group=64, topk_group=9, renormalize=True, scale=1.5, stats=True)
    _forward_checks(res, want, "64 groups, K = 17")
    # the bias has no gradient and steers the choice only: the weights are the scores, not c
    bias = torch.tensor([0.0, 0.0, 5.0, 0.0]).requires_grad_(True)
    res = route_topk_grouped(torch.tensor([[3.0, 2.0, -1.0, 0.0]], requires_grad=True), 2, bias=bias)
    assert res.ids.tolist() == [[2, 0]] and abs(float(res.weights.detach()[0, 0]) - 0.2689414) < 1e-6
    res.weights.sum().backward()
    assert bias.grad is None
