#!/usr/bin/env python3
"""The group-limited router gate on one GPU, one process per row:

fused    K13 (csrc/kernels/moe_gate_group.hip) through ``route_topk_grouped``: sigmoid score, selection
         bias, ``n_group`` groups of which ``topk_group`` are used, renormalisation, scale 2.5
torch    the same definition as a user writes it today: ``gate_group_forward_torch`` /
         ``gate_group_backward_torch`` on the same GPU tensors (not the code under test)
plain    K13 with one group, no bias and the softmax score, next to
k10      K10 (``route_topk``) on the same logits: the difference is the cost of the group step

Per shape (T tokens x E experts, Gr groups, Kg used, top K, logits dtype): the forward alone and
forward + backward (the gradient of the gate weights fed back, the logits' gradient out).  A call is
timed as a batch of ``--iters`` launches between two device events; the forms alternate in
``--rounds`` rounds and a row gives the median of the rounds with their extremes.  Every row runs in
a child process under its own time limit, and the first failure ends the run.  Prints one JSON line
per row and form."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((256, 8, 4, 8), (64, 8, 3, 6))
DTYPES = ("bfloat16", "float32")
SCALE = 2.5


def _batch_us(torch, call, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        call()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / iters


def row(a, E, Gr, Kg, K, dtype):
    import torch
    from mp4x.models.moe import (gate_group_backward_torch, gate_group_forward_torch, route_topk, route_topk_grouped)
    if not torch.cuda.is_available():
        raise SystemExit("bench/moe_router_group.py needs a GPU")
    torch.cuda.set_device(0)
    T, dt = a.tokens, getattr(torch, dtype)
    g = torch.Generator(device="cuda").manual_seed(E * 100 + K)
    logits = torch.randn(T, E, device="cuda", generator=g).to(dt).requires_grad_(True)
    plain = logits.detach()
    bias = (torch.rand(E, device="cuda", generator=g) - 0.5) * 0.2
    gw = torch.randn(T, K, device="cuda", generator=g)
    kw = dict(score="sigmoid", bias=bias, n_group=Gr, topk_group=Kg, renormalize=True, scale=SCALE)

    def fused_fwd():
        return route_topk_grouped(plain, K, **kw)

    def fused_fb():
        logits.grad = None
        route_topk_grouped(logits, K, **kw).weights.backward(gw)

    def torch_fwd():
        return gate_group_forward_torch(plain, K, "sigmoid", bias, Gr, Kg, True, SCALE, torch.int64, False)

    def torch_fb():
        w, ids, lse, _, _, _ = gate_group_forward_torch(plain, K, "sigmoid", bias, Gr, Kg, True, SCALE, torch.int64, False)
        return gate_group_backward_torch(plain, lse, ids, "sigmoid", True, SCALE, gw, None, None)

    def plain_fwd():
        return route_topk_grouped(plain, K, score="softmax", renormalize=True)

    def plain_fb():
        logits.grad = None
        route_topk_grouped(logits, K, score="softmax", renormalize=True).weights.backward(gw)

    def k10_fwd():
        return route_topk(plain, K, True)

    def k10_fb():
        logits.grad = None
        route_topk(logits, K, True).weights.backward(gw)

    same = float((fused_fwd().ids == torch_fwd()[1]).float().mean())
    forms = (("fused", "forward", fused_fwd), ("fused", "forward + backward", fused_fb), ("torch", "forward", torch_fwd),
             ("torch", "forward + backward", torch_fb), ("plain", "forward", plain_fwd),
             ("plain", "forward + backward", plain_fb), ("k10", "forward", k10_fwd), ("k10", "forward + backward", k10_fb))
    for _, _, call in forms:
        for _ in range(5):
            call()
    torch.cuda.synchronize()
    us = {f[:2]: [] for f in forms}
    for _ in range(a.rounds):                    # the forms alternate: a drifting clock hits all of them
        for form, phase, call in forms:
            us[(form, phase)].append(_batch_us(torch, call, a.iters))
    for form, phase, _ in forms:
        v = sorted(us[(form, phase)])
        print(json.dumps({"gpus": 1, "tokens": T, "experts": E, "n_group": Gr, "topk_group": Kg, "top_k": K, "dtype": dtype,
                          "form": form, "phase": phase, "us_median_of_rounds": round(v[len(v) // 2], 2),
                          "min_of_rounds": round(v[0], 2), "max_of_rounds": round(v[-1], 2),
                          "ids_equal_torch_form": round(same, 6),
                          "timed": f"{a.iters} launches between two device events, host launch cost included"}),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=16384)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--row-timeout", type=float, default=120.0, help="seconds a row's process may take")
    ap.add_argument("--row", default=None, help="E,Gr,Kg,K,dtype: run this row in this process")
    a = ap.parse_args()
    if a.row:
        E, Gr, Kg, K, dtype = a.row.split(",")
        row(a, int(E), int(Gr), int(Kg), int(K), dtype)
        return
    for dtype in DTYPES:
        for shape in SHAPES:
            spec = ",".join(str(v) for v in shape) + "," + dtype
            cmd = [sys.executable, os.path.abspath(__file__), "--row", spec, "--tokens", str(a.tokens), "--iters",
                   str(a.iters), "--rounds", str(a.rounds)]
            try:
                rc = subprocess.run(cmd, timeout=a.row_timeout).returncode
            except subprocess.TimeoutExpired:
                raise SystemExit(f"row {spec}: not done after {a.row_timeout} s; the run ends here")
            if rc != 0:
                raise SystemExit(f"row {spec}: exit status {rc}; the run ends here")


if __name__ == "__main__":
    main()
