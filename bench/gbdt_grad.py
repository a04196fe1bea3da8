#!/usr/bin/env python3
"""K21 on one process and one GPU: the two loss kernels of a boosting round (``device_ops.gbdt_grad_absmax``, then
``device_ops.gbdt_grad_quantize``) against (a) the torch chain they replace - the definition ``gbdt_grad_torch`` on GPU
tensors, ``abs().max()`` of ``g`` and of ``h`` per class, and K16's ``gbdt_quantize`` per class - and (b) a plain device
copy of the bytes the two kernels must move (``2 (8 C + 8) n`` read, ``8 C n`` written: the copy reads and writes ``(12
C + 8) n``), alternating in one process.  ``C = 1`` is the logistic loss, ``C > 1`` softmax.

The chain's ``gh`` and maxima are compared with the kernels' bit for bit first, at the timed size (a NaN maximum
equal to any NaN).  Device-event times, one warm-up of every arm, ``--rounds`` rounds of three calls (one of the
torch chain); medians and min-max.  One JSON line per shape.

Usage: python bench/gbdt_grad.py [--rounds 5] [--out FILE] [--quick]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def timed(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(reps)]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="one small shape: a rehearsal of the script")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench/gbdt_grad.py measures on a GPU; none is visible")
    from mp4x.ops import device_ops
    from mp4x.parallel.gbdt import gbdt_grad_torch
    dev = torch.device("cuda", 0)
    shapes = [(1 << 14, 3)] if a.quick else [(n, C) for n in (1 << 20, 1 << 23) for C in (1, 8, 32)]
    lines = []
    for n, C in shapes:
        loss = "softmax" if C > 1 else "logistic"
        gen = torch.Generator(device=dev).manual_seed(n + C)
        pred = torch.randn((C, n) if C > 1 else (n,), dtype=torch.float64, device=dev, generator=gen) * 4
        y = torch.randint(0, max(C, 2), (n,), device=dev, generator=gen)
        y = y if C > 1 else y.double()
        sg = torch.full((C,), 29, dtype=torch.int32, device=dev)
        sh = torch.full((C,), 31, dtype=torch.int32, device=dev)
        top = torch.empty(C, 2, dtype=torch.float32, device=dev)
        gh = torch.empty(C, n, 2, dtype=torch.int32, device=dev)
        moved = (12 * C + 8) * n
        src = torch.empty(moved, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        kept = {}

        def kernels():
            device_ops.gbdt_grad_absmax(pred, y, loss, out=top)
            device_ops.gbdt_grad_quantize(pred, y, loss, sg, sh, out=gh)

        def chain():
            g, h = (t.reshape(C, n) for t in gbdt_grad_torch(pred, y, loss))
            kept["top"] = torch.stack([g.abs().max(dim=1).values, h.abs().max(dim=1).values], dim=1)
            kept["gh"] = torch.stack([device_ops.gbdt_quantize(g[c], h[c], 29, 31) for c in range(C)])

        runs = {"kernels": kernels, "torch": chain, "copy": lambda: dst.copy_(src)}
        for fn in runs.values():           # warm up every arm; the results of this pass are the ones compared
            fn()
        torch.cuda.synchronize()
        same = torch.equal(gh, kept["gh"]) and torch.equal(top.isnan(), kept["top"].isnan()) and \
            torch.equal(top.nan_to_num(nan=0.0), kept["top"].nan_to_num(nan=0.0))
        kept.clear()
        times = {name: [] for name in runs}
        for _ in range(a.rounds):          # alternate, so drift hits every arm alike
            for name, fn in runs.items():
                times[name] += timed(fn, 1 if name == "torch" else 3)
                kept.clear()
        med = {name: statistics.median(t) for name, t in times.items()}
        line = dict(n=n, C=C, loss=loss, same_bits=same, bytes=2 * moved,
                    ms={name: round(v, 4) for name, v in med.items()},
                    ms_min_max={name: [round(min(t), 4), round(max(t), 4)] for name, t in times.items()},
                    kernels_vs_torch=round(med["torch"] / med["kernels"], 2),
                    kernels_GBps=round(2 * moved / med["kernels"] / 1e6, 1), copy_GBps=round(2 * moved / med["copy"] / 1e6, 1),
                    fraction_of_copy=round(med["copy"] / med["kernels"], 3))
        lines.append(line)
        print(json.dumps(line), flush=True)
        del pred, y, gh, src, dst
    if a.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(x) for x in lines) + "\n")
    return 0 if all(x["same_bits"] for x in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
