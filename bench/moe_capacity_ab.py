#!/usr/bin/env python3
"""A/B of the K9 route scatter under an expert capacity, one process on GPU 0: this tree's unclipped
entry point, the clipped entry point with a quota that clips nothing, and the clipped entry point at
capacity factors 1.0 / 0.5 / 0.25 / 0.125 (C = ceil(f * n / E) on this call's ids, top-k of random
logits); with --parent-lib, also the unclipped entry point of another build of libmp4x_hip.so (the
commit before the capacity) loaded next to this one.  Default shape: bf16, 4096 x 7168, K = 8, 64
experts.  The variants alternate in rounds; every call is timed with device events; a row gives
the median, minimum and maximum of the rounds' p50s, the bytes the variant must move (token rows
read + rows written + ids and slots) and whether its slots and rows equal the first variant's bit
for bit.  Then the upload of the quota table two ways (host clock around 200 uploads ending in a
device synchronise).  Prints one JSON line per row."""
import argparse
import ctypes
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mp4x.ops import device_ops as ops, native  # noqa: E402
from mp4x.ops.hip_sigs import HIP_SIGS  # noqa: E402
from mp4x.parallel.moe import capacity_quota  # noqa: E402

BF16 = int(ops.dtype_of_torch(torch.bfloat16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="another build of libmp4x_hip.so to time next to this one")
    ap.add_argument("--tokens", type=int, default=4096)
    ap.add_argument("--width", type=int, default=7168)
    ap.add_argument("--top-k", type=int, default=8)
    ap.add_argument("--experts", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    TOKENS, WIDTH, K, E, ROUNDS, ITERS = a.tokens, a.width, a.top_k, a.experts, a.rounds, a.iters
    torch.cuda.set_device(0)
    lib = native.hip()
    g = torch.Generator(device="cuda").manual_seed(900)
    x = torch.randn(TOKENS, WIDTH, device="cuda", generator=g).to(torch.bfloat16)
    logits = torch.randn(TOKENS, E, device="cuda", generator=g)
    _, ids = torch.topk(torch.softmax(logits, -1), K, dim=-1)
    flat = ids.reshape(-1).contiguous()
    n, rb = flat.numel(), WIDTH * 2
    rc = ops.moe_route_count(flat, E)
    demand = rc.counts[:E].tolist()
    FACTORS = (1.0, 0.5, 0.25, 0.125)
    caps = {f: max(1, math.ceil(f * n / E)) for f in FACTORS}

    def table(keep):
        base, tot = [], 0
        for k in keep:
            base.append(tot)
            tot += k
        return torch.tensor(list(keep) + base, dtype=torch.int64, device="cuda"), tot

    clip_all, kept_all = table(demand)
    clips = {f: table(list(capacity_quota([demand], caps[f])[0])) for f in FACTORS}
    assert kept_all == n
    rows = torch.empty(n, WIDTH, dtype=torch.bfloat16, device="cuda")
    slots = torch.empty(n, dtype=torch.int64, device="cuda")
    head = (BF16, flat.data_ptr(), 1, x.data_ptr(), None, n, K, rb, E, rows.data_ptr(), slots.data_ptr())
    tail = (rc.scratch.data_ptr(), rc.scratch.numel(), None)

    def chk(code):
        assert code == 0, code

    variants = {}
    if a.parent_lib:
        parent = ctypes.CDLL(a.parent_lib, mode=ctypes.RTLD_LOCAL)
        res, args = HIP_SIGS["mp4x_moe_route_scatter"]
        parent.mp4x_moe_route_scatter.restype, parent.mp4x_moe_route_scatter.argtypes = res, args
        variants["parent"] = (lambda: chk(parent.mp4x_moe_route_scatter(*head, *tail)), n)
    variants.update({
        "unclipped": (lambda: chk(lib.mp4x_moe_route_scatter(*head, *tail)), n),
        "clip_nothing": (lambda: chk(lib.mp4x_moe_route_scatter_clip(*head, clip_all.data_ptr(), *tail)), n),
    })
    first = next(iter(variants))
    for f in FACTORS:
        variants[f"clip_f{f}"] = ((lambda t=clips[f][0]: chk(lib.mp4x_moe_route_scatter_clip(*head, t.data_ptr(), *tail))),
                                  clips[f][1])
    # results first: the same bits where the same rows are kept
    outs = {}
    for name, (call, kept) in variants.items():
        rows.fill_(0)
        slots.fill_(-7)
        call()
        torch.cuda.synchronize()
        outs[name] = (slots.clone(), rows[:kept].clone())
    same = {name: bool(torch.equal(outs[name][0], outs[first][0])
                       and torch.equal(outs[name][1].view(torch.int16), outs[first][1].view(torch.int16)))
            for name in ("unclipped", "clip_nothing") if name != first}
    kept_tokens = {}
    for f in FACTORS:
        s1 = outs[f"clip_f{f}"][0]
        kept_tokens[f"clip_f{f}"] = int((s1.view(TOKENS, K) >= 0).any(1).sum())
        assert int((s1 >= 0).sum()) == clips[f][1]

    p50s = {name: [] for name in variants}
    for name, (call, _) in variants.items():                        # warm up every variant
        for _ in range(5):
            call()
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for name, (call, _) in variants.items():
            s = [torch.cuda.Event(enable_timing=True) for _ in range(ITERS)]
            e = [torch.cuda.Event(enable_timing=True) for _ in range(ITERS)]
            for i in range(ITERS):
                s[i].record()
                call()
                e[i].record()
            torch.cuda.synchronize()
            ts = sorted(a.elapsed_time(b) for a, b in zip(s, e))
            p50s[name].append(ts[len(ts) // 2] * 1e3)
    with open(a.out or os.devnull, "w") as f:
        for name, (_, kept) in variants.items():
            v = sorted(p50s[name])
            nbytes = kept_tokens.get(name, TOKENS) * rb + kept * rb + n * 16
            row = {"variant": name, "rows_kept": kept, "of": n, "token_rows_read": kept_tokens.get(name, TOKENS),
                   "capacity": caps.get(float(name[6:])) if name.startswith("clip_f") else None,
                   "bytes": nbytes, "p50_us_median_of_rounds": round(v[len(v) // 2], 1), "min": round(v[0], 1),
                   "max": round(v[-1], 1), "rounds": [round(t, 1) for t in p50s[name]],
                   "eff_gbps": round(nbytes / v[len(v) // 2] / 1e3, 1), f"same_bits_as_{first}": same.get(name)}
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + "\n")
        # the table's upload, host clock around 200 uploads each ending in a device synchronise
        import time
        vals = clips[1.0][0].tolist()
        forms = {"pageable": lambda: torch.tensor(vals, dtype=torch.int64).to("cuda"),
                 "pinned_async": lambda: torch.tensor(vals, dtype=torch.int64).pin_memory().to("cuda", non_blocking=True)}
        for name, up in forms.items():
            for _ in range(10):
                up()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(200):
                t = up()
            torch.cuda.synchronize()
            row = {"upload": name, "us_per_call": round((time.perf_counter() - t0) / 200 * 1e6, 1),
                   "same": bool(torch.equal(t, clips[1.0][0]))}
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
