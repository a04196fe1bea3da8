#!/usr/bin/env python3
"""Drop by gate weight (K15) on one GPU, one process: what a priority dispatch adds to the position
call's local half.  No expert GEMM, no layer step, no second rank.

added     ``moe_priority_mask`` + the second ``moe_route_count`` (on the masked ids): everything a
          padded priority dispatch runs that the position call does not
mask      ``moe_priority_mask`` alone
torch     ``priority_mask_torch`` (the definition: two stable sorts) on the same GPU tensors
position  the position call's local half: ``moe_route_count`` + ``moe_pad_counts`` +
          ``moe_route_scatter_pad`` (scatter and pad fill) on the caller's ids
position2 the same call again: timed twice, so the spread of one form is next to the differences
          between forms.  ``--only-position`` times these two alone; it uses nothing of K15, so the
          same file runs from a checkout of the commit before K15 to show the position path did not move

Shapes: T tokens x K = 8 assignments, E experts, bf16 rows of ``--width`` elements; the share S is
the median per-expert count, so about half the experts overflow.  Id distributions: ``uniform``;
``skewed`` (expert e drawn with weight 1 / (e + 1)); ``one`` (every assignment to expert 0: one block
of the select walks all T*K words eight times).  A form is timed as a batch of ``--iters`` calls
between two device events; the forms alternate in ``--rounds`` rounds; a row gives the median of the
rounds with their extremes.  Prints one JSON line per (E, distribution, form)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EXPERTS = (64, 256)
DISTS = ("uniform", "skewed", "one")
TOP_K = 8


def _batch_us(torch, call, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        call()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / iters


def _ids(torch, dist, T, E, g):
    n = T * TOP_K
    if dist == "uniform":
        return torch.randint(0, E, (n,), device="cuda", generator=g)
    if dist == "skewed":
        w = 1.0 / torch.arange(1, E + 1, device="cuda", dtype=torch.float32)
        return torch.multinomial(w, n, replacement=True, generator=g)
    return torch.zeros(n, dtype=torch.int64, device="cuda")


def row(a, E, dist):
    import torch
    from mp4x.ops import device_ops as ops
    if not torch.cuda.is_available():
        raise SystemExit("bench/moe_priority.py needs a GPU")
    torch.cuda.set_device(0)
    T, n = a.tokens, a.tokens * TOP_K
    g = torch.Generator(device="cuda").manual_seed(E + len(dist))
    ids = _ids(torch, dist, T, E, g)
    prio = torch.rand(n, device="cuda", generator=g)
    x = torch.randn(T, a.width, device="cuda", generator=g).to(torch.bfloat16)
    counts = torch.bincount(ids, minlength=E)
    S = max(1, int(counts.float().median()))
    over = int((counts > S).sum())
    send = torch.empty((E * S, a.width), dtype=torch.bfloat16, device="cuda")

    def position():
        rc = ops.moe_route_count(ids, E)
        ops.moe_pad_counts(rc, S)
        ops.moe_route_scatter_pad(rc, x, TOP_K, send, S)

    forms = [("position", position), ("position2", position)]
    same = None
    if not a.only_position:
        from mp4x.parallel.moe import priority_mask_torch
        rc0 = ops.moe_route_count(ids, E)

        def mask():
            return ops.moe_priority_mask(rc0, prio, S)

        def added():
            ops.moe_route_count(ops.moe_priority_mask(rc0, prio, S)[0], E)

        def torch_form():
            return priority_mask_torch(ids, prio, E, S)

        same = bool(torch.equal(mask()[0], torch_form()[0])) and bool(torch.equal(mask()[1], torch_form()[1]))
        forms += [("added", added), ("mask", mask), ("torch", torch_form)]
    for _, call in forms:
        for _ in range(5):
            call()
    torch.cuda.synchronize()
    us = {f: [] for f, _ in forms}
    for _ in range(a.rounds):                    # the forms alternate: a drifting clock hits all of them
        for form, call in forms:
            us[form].append(_batch_us(torch, call, a.iters))
    med = {}
    for form, _ in forms:
        v = sorted(us[form])
        med[form] = v[len(v) // 2]
        rec = {"gpus": 1, "tokens": T, "top_k": TOP_K, "experts": E, "ids": dist, "share": S, "experts_over": over,
               "width": a.width, "form": form, "us_median_of_rounds": round(med[form], 2), "min_of_rounds": round(v[0], 2),
               "max_of_rounds": round(v[-1], 2),
               "timed": f"{a.iters} calls between two device events, host launch cost included"}
        if form == "added":
            rec["added_over_position"] = round(med["added"] / med["position"], 3)
            rec["mask_equals_torch_form"] = same
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=16384)
    ap.add_argument("--width", type=int, default=1024, help="elements of a bf16 token row")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only-position", action="store_true", help="time the position call's local half alone")
    a = ap.parse_args()
    for E in EXPERTS:
        for dist in DISTS:
            row(a, E, dist)


if __name__ == "__main__":
    main()
