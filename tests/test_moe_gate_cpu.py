"""The router gate on the CPU (mp4x/models/moe.py: ``route_topk``, its torch form and its closed-form
backward) against the float64 definition of tests/moe_gate_ref.py: the ids exactly (ties, masks,
16-bit logits), weights / lse / prob_sum and the gradient inside the derived bounds (DESIGN "K10":
B = (2R + E/16 + 16) u forward, 4 (B + K u) p_j (A_j + sum_i A_i p_i + |g_lse|) backward, plus one
rounding to a 16-bit dtype), counts exactly.

The 16-bit rounding term is the format's unit roundoff, 2^-8 (bfloat16) / 2^-11 (float16) of |g64|,
plus 2^-25 absolute for float16 (half a subnormal step, where no relative bound can hold).  The
issue's first figures for it, 2^-9 / 2^-12, are half of that: torch's own float32 evaluation of
the closed form, rounded once to bfloat16, reached 1.95 of the bound built with them (E = 257,
K = 16, only g_psum present), so the derivation was corrected here and in DESIGN."""
import pytest

torch = pytest.importorskip("torch")

import moe_gate_ref as ref  # noqa: E402
from mp4x.models.moe import gate_backward_torch, gate_forward_torch, route_topk  # noqa: E402

T = 65
ES, KS = (2, 5, 64, 257, 2048), (1, 2, 8, 16)


def _forward_checks(res, want, what):
    assert torch.equal(res.ids.to(torch.int64), want.ids), (what, "ids")
    for name, got, w64, bound in (("weights", res.weights, want.w, want.weights_bound()),
                                  ("lse", res.lse, want.lse, want.lse_bound()),
                                  ("prob_sum", res.prob_sum, want.prob_sum, want.prob_sum_bound())):
        ok, ratio = ref.inside(got, w64, bound)
        print(what, name, "worst / bound = %.3f" % ratio)
        assert ok, (what, name, ratio)
    assert torch.equal(res.counts, want.counts), (what, "counts")


@pytest.mark.parametrize("renormalize", [False, True])
@pytest.mark.parametrize("R", [4, 32])
@pytest.mark.parametrize("E", ES)
def test_forward_and_backward_inside_the_bounds(E, R, renormalize):
    for K in sorted({min(k, E) for k in KS}):
        logits, want = ref.cached_reference("uniform", T, E, K, renormalize, R, 100 + E + K, "float32")
        lg = logits.clone().requires_grad_(True)
        res = route_topk(lg, K, renormalize, stats=True)
        _forward_checks(res, want, (E, K, R, renormalize))
        assert res.weights.requires_grad and res.lse.requires_grad and res.prob_sum.requires_grad
        assert not res.ids.requires_grad and not res.counts.requires_grad
        grads = ref.gradients(T, E, K, 200 + E + K)
        g64, bound = want.backward(*grads)
        (res.weights * grads[0]).sum().add((res.lse * grads[1]).sum()).add((res.prob_sum * grads[2]).sum()).backward()
        ok, ratio = ref.inside(lg.grad, g64, bound)
        print((E, K, R, renormalize), "g_logits worst / bound = %.3f" % ratio)
        assert ok, (E, K, R, renormalize, ratio)


@pytest.mark.parametrize("renormalize", [False, True])
@pytest.mark.parametrize("which", ref.GRAD_SETS)
def test_backward_with_every_combination_of_absent_gradients(which, renormalize):
    for E, K, dtype in ((5, 2, "float32"), (64, 8, "float32"), (257, 16, "bfloat16"), (64, 2, "float16")):
        logits, want = ref.cached_reference("uniform", T, E, K, renormalize, 4, 300 + E, dtype)
        grads = ref.pick(ref.gradients(T, E, K, 400 + E), which)
        g64, bound = want.backward(*grads)
        # the closed form, called directly with None for an absent gradient ...
        w, ids, lse, _, _ = gate_forward_torch(logits, K, renormalize, torch.int64, False)
        got = gate_backward_torch(logits, lse, ids, renormalize, *grads)
        assert got.dtype == logits.dtype
        ok, ratio = ref.inside(got, g64, bound)
        assert ok, (E, K, dtype, which, ratio)
        # ... and through autograd, where an unused output's gradient is absent
        lg = logits.clone().requires_grad_(True)
        res = route_topk(lg, K, renormalize, stats=True)
        terms = [(o * g).sum() for o, g in zip((res.weights, res.lse, res.prob_sum), grads) if g is not None]
        if terms:
            sum(terms).backward()
            ok, ratio = ref.inside(lg.grad, g64, bound)
            assert ok, (E, K, dtype, which, "autograd", ratio)
        else:
            assert not bool(got.to(torch.float32).abs().max() > 0)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("E", [1, 2, 5, 64, 257])
def test_ids_on_ties_and_masks_equal_the_stable_sort(E, dtype):
    for K in sorted({min(k, E) for k in KS}):
        for renormalize in (False, True):
            logits, want = ref.cached_reference("ties", T, E, K, renormalize, 0, 500 + E, dtype)
            for ids_dtype in (torch.int64, torch.int32):
                res = route_topk(logits, K, renormalize, ids_dtype=ids_dtype, stats=True)
                assert res.ids.dtype == ids_dtype
                _forward_checks(res, want, (E, K, dtype, renormalize))
    # -inf is chosen only after every finite logit, in index order
    lg = torch.tensor([[float("-inf"), 0.0, float("-inf"), -0.0, 1.0]])
    res = route_topk(lg, 5)
    assert res.ids.tolist() == [[4, 1, 3, 0, 2]] and res.weights[0, 3:].tolist() == [0.0, 0.0]


def test_empty_and_refusals():
    for stats in (False, True):
        res = route_topk(torch.empty(0, 7, requires_grad=True), 3, stats=stats)
        assert res.weights.shape == (0, 3) and res.ids.shape == (0, 3) and res.lse.shape == (0,)
        if stats:
            assert res.prob_sum.tolist() == [0.0] * 7 and res.counts.tolist() == [0] * 7
        else:
            assert res.prob_sum is None and res.counts is None
    for bad in (0, 8, True, 2.0):
        with pytest.raises(ValueError):
            route_topk(torch.zeros(3, 7), bad)
    with pytest.raises(ValueError):
        route_topk(torch.zeros(3, 7), 2, ids_dtype=torch.int16)
    with pytest.raises(ValueError):
        route_topk(torch.zeros(7), 1)
    # outside the kernel's range the same definition runs in torch: K = 17, E = 2049
    lg = ref.uniform_logits(3, 2049, 4, 9)
    res = route_topk(lg, 17, True, stats=True)
    want = ref.Reference(lg, 17, True)
    _forward_checks(res, want, "E = 2049, K = 17")
