#!/usr/bin/env python3
"""The MoE router gate two ways on one GPU, one process:

fused   K10 (csrc/kernels/moe_gate.hip) through ``route_topk``: one kernel forward, one backward
torch   ``softmax`` (float32) + ``topk`` with torch autograd, the router of ``ExpertParallelMoE.route()``
copy    a plain device copy of the logits' bytes (read them, write as many): the roofline of a pass

Per shape (T tokens x E experts, top K, logits dtype): the forward alone, forward + backward (the
gradient of the gate weights fed back, the logits' gradient out), and for K10 the forward with the
router statistics.  A call is timed as a batch of ``--iters`` launches between two device events; the
forms alternate in ``--rounds`` rounds and a row gives the median of the rounds with their extremes.
``bytes`` is what one pass has to move (the logits once, plus the logits' gradient for the backward;
the [T, K] outputs are left out).  ``--profile`` runs only the K10 launches, a few times, for a
kernel trace.  Prints one JSON line per row."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _batch_us(torch, call, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        call()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=16384)
    ap.add_argument("--experts", default="8,64,256")
    ap.add_argument("--top-k", default="2,8")
    ap.add_argument("--dtypes", default="float32,bfloat16")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--profile", action="store_true", help="only the K10 launches, 5 of each: for a kernel trace")
    a = ap.parse_args()
    import torch
    from mp4x.models.moe import route_topk
    if not torch.cuda.is_available():
        raise SystemExit("bench/moe_router.py needs a GPU")
    torch.cuda.set_device(0)
    T = a.tokens
    for dtype in a.dtypes.split(","):
        dt = getattr(torch, dtype)
        for E in (int(x) for x in a.experts.split(",")):
            for K in (int(x) for x in a.top_k.split(",")):
                g = torch.Generator(device="cuda").manual_seed(E * 100 + K)
                logits = torch.randn(T, E, device="cuda", generator=g).to(dt).requires_grad_(True)
                plain = logits.detach()
                gw = torch.randn(T, K, device="cuda", generator=g)
                dst = torch.empty_like(plain)

                def fused_fwd():
                    return route_topk(plain, K)

                def fused_stats():
                    return route_topk(plain, K, stats=True)

                def fused_fb():
                    logits.grad = None
                    route_topk(logits, K).weights.backward(gw)

                def torch_fwd():
                    return torch.topk(torch.softmax(plain.to(torch.float32), dim=-1), K, dim=-1)

                def torch_fb():
                    logits.grad = None
                    torch.topk(torch.softmax(logits.to(torch.float32), dim=-1), K, dim=-1)[0].backward(gw)

                def copy():
                    dst.copy_(plain)

                if a.profile:
                    for call in (fused_fwd, fused_stats, fused_fb):
                        for _ in range(5):
                            call()
                    torch.cuda.synchronize()
                    continue
                # the two forms choose the same experts wherever the probabilities are distinct
                same = float((fused_fwd().ids == torch_fwd()[1]).float().mean())
                nb = plain.numel() * plain.element_size()
                forms = (("fused", "forward", fused_fwd, nb), ("fused", "forward + statistics", fused_stats, nb),
                         ("fused", "forward + backward", fused_fb, 3 * nb), ("torch", "forward", torch_fwd, nb),
                         ("torch", "forward + backward", torch_fb, 3 * nb), ("copy", "read + write", copy, 2 * nb))
                for _, _, call, _ in forms:
                    for _ in range(5):
                        call()
                torch.cuda.synchronize()
                us = {f[:2]: [] for f in forms}
                for _ in range(a.rounds):                    # the forms alternate: a drifting clock hits all of them
                    for form, phase, call, _ in forms:
                        us[(form, phase)].append(_batch_us(torch, call, a.iters))
                for form, phase, _, nbytes in forms:
                    v = sorted(us[(form, phase)])
                    med = v[len(v) // 2]
                    print(json.dumps({"gpus": 1, "tokens": T, "experts": E, "top_k": K, "dtype": dtype, "form": form,
                                      "phase": phase, "us_median_of_rounds": round(med, 2), "min_of_rounds": round(v[0], 2),
                                      "max_of_rounds": round(v[-1], 2), "bytes": nbytes,
                                      "eff_gbps": round(nbytes / med / 1e3, 1), "ids_equal_torch_topk": round(same, 6),
                                      "timed": f"{a.iters} launches between two device events, host launch cost included"}),
                          flush=True)


if __name__ == "__main__":
    main()
