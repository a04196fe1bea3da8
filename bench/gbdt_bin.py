#!/usr/bin/env python3
"""K19 on one process and one GPU: the binning kernel (``device_ops.gbdt_bin``) against (a) a torch form of the
same definition on the GPU - the features transposed, one batched ``torch.searchsorted(right=True)`` over the
ascending edges, clamped to ``cnt``, NaN to ``missing``, transposed back to bytes - and (b) a plain device copy
that moves as many bytes (``4 n F`` read and ``n F`` written by the kernel; the copy reads and writes ``2.5 n F``),
alternating in one process.  There is no earlier GPU binning to compare with.

The edges are ``gbdt_edges`` of the first 65536 rows; one value in 128 is NaN.  The kernel's and the torch form's
bins are compared bit for bit first, at the timed size.  Device-event times, one warm-up of every arm,
``--rounds`` rounds of three calls (one of the torch form); medians and min-max.  One JSON line per shape.

Usage: python bench/gbdt_bin.py [--rounds 5] [--out FILE] [--quick]
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


def torch_form(X, edges, cnt, missing):
    """The definition for ascending edges padded with ``+inf`` and finite or NaN values, in plain torch."""
    Xt = X.t().contiguous()
    pos = torch.searchsorted(edges, Xt, right=True, out_int32=True)
    pos = torch.minimum(pos, cnt[:, None])
    return torch.where(Xt.isnan(), missing, pos).to(torch.uint8).t().contiguous()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="one small shape: a rehearsal of the script")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench/gbdt_bin.py measures on a GPU; none is visible")
    from mp4x.ops import device_ops
    from mp4x.parallel.gbdt import gbdt_edges
    dev = torch.device("cuda", 0)
    shapes = [(1 << 14, 28, 64)] if a.quick else \
        [(n, F, B) for n in (1 << 20, 1 << 23) for F in (28, 128) for B in (64, 256)]
    missing, lines = 255, []
    for n, F, B in shapes:
        gen = torch.Generator(device=dev).manual_seed(n + F + B)
        X = torch.randn(n, F, device=dev, generator=gen)
        X[torch.rand(n, F, device=dev, generator=gen) < 1 / 128] = float("nan")
        edges, cnt = gbdt_edges(None, X[:65536], B)
        out = torch.empty(n, F, dtype=torch.uint8, device=dev)
        src = torch.empty(n * F * 5 // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        kept = {}
        runs = {"kernel": lambda: device_ops.gbdt_bin(X, edges, cnt, missing, out=out),
                "torch": lambda: kept.update(torch=torch_form(X, edges, cnt, missing)),
                "copy": lambda: dst.copy_(src)}
        for fn in runs.values():           # warm up every arm; the results of this pass are the ones compared
            fn()
        torch.cuda.synchronize()
        same = torch.equal(out, kept["torch"])
        times = {name: [] for name in runs}
        for _ in range(a.rounds):          # alternate, so drift hits every arm alike
            for name, fn in runs.items():
                times[name] += timed(fn, 1 if name == "torch" else 3)
        med = {name: statistics.median(t) for name, t in times.items()}
        line = dict(n=n, F=F, B=B, edges_min_max=[int(cnt.min()), int(cnt.max())], same_bits=same, bytes=5 * n * F,
                    ms={name: round(v, 4) for name, v in med.items()},
                    ms_min_max={name: [round(min(t), 4), round(max(t), 4)] for name, t in times.items()},
                    kernel_vs_torch=round(med["torch"] / med["kernel"], 2),
                    kernel_GBps=round(5 * n * F / med["kernel"] / 1e6, 1), copy_GBps=round(5 * n * F / med["copy"] / 1e6, 1),
                    fraction_of_copy=round(med["copy"] / med["kernel"], 3))
        lines.append(line)
        print(json.dumps(line), flush=True)
        del X, out, src, dst, kept
    if a.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(x) for x in lines) + "\n")
    return 0 if all(x["same_bits"] for x in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
