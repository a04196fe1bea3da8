#!/usr/bin/env python3
"""K16 A/B on one process and one GPU: ``device_ops.gbdt_histogram`` against the torch form of the same
definition on the GPU (``index_add_`` into an int64 ``[k * F * B, 2]``, one feature at a time so the index
tensor stays ``[m]``), which is what the kernel replaces.  Per shape the two alternate for ``--rounds``
rounds; the medians of device-event times are reported with the achieved bytes/s of ``bins + gh + rows``
against a plain copy of as many bytes in the same run.  The results are compared bit for bit first.
Also timed: quantise, split and the row multisplit, for the histogram's share of a tree level.
Nothing here runs two ranks on one GPU or more than one GPU.  One JSON line per shape.

Usage: python bench/gbdt_hist.py [--rounds 7] [--out FILE] [--quick]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def torch_hist(bins, gh, rows, seg, B):
    """The definition with torch GPU ops (benign tables only: seg is the true offsets)."""
    n, F = bins.shape
    k = seg.numel() - 1
    r = rows.to(torch.int64)
    node = torch.searchsorted(seg[1:].contiguous(), torch.arange(r.numel(), device=r.device), right=True)
    val = gh[r].to(torch.int64)
    hist = torch.zeros(k * F * B, 2, dtype=torch.int64, device=bins.device)
    for f in range(F):
        hist.index_add_(0, (node * F + f) * B + bins[r, f].to(torch.int64), val)
    return hist.view(k, F, B, 2)


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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="one small shape: a rehearsal of the script")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench/gbdt_hist.py measures on a GPU; none is visible")
    from mp4x.ops import device_ops
    from mp4x.parallel import gbdt
    dev = torch.device("cuda", 0)
    shapes = [(1 << 16, 28, 8, "uniform")] if a.quick else \
        [(n, F, k, dist) for n in (1 << 20, 1 << 23) for F in (28, 128) for k in (1, 8, 32) for dist in ("uniform", "skewed")]
    B, lines = 256, []
    for n, F, k, dist in shapes:
        gen = torch.Generator(device=dev).manual_seed(n + F + k)
        bins = torch.randint(0, B, (n, F), dtype=torch.uint8, device=dev, generator=gen)
        if dist == "skewed":       # one column with 95 % of its rows in one bin
            bins[:, 0] = torch.where(torch.rand(n, device=dev, generator=gen) < 0.95, 7, bins[:, 0].to(torch.int64)).to(torch.uint8)
        g, h = torch.randn(n, device=dev, generator=gen), torch.ones(n, device=dev)
        node = torch.randint(0, k, (n,), device=dev, generator=gen)
        slot_of_node = torch.arange(k, device=dev)
        rows, seg = gbdt.gbdt_level_rows(node, slot_of_node, k)
        sg, sh = gbdt.gbdt_shift(float(g.abs().max())), gbdt.gbdt_shift(1.0)
        gh = device_ops.gbdt_quantize(g, h, sg, sh)
        hist = torch.empty(k, F, B, 2, dtype=torch.int64, device=dev)
        device_ops.gbdt_histogram(bins, gh, rows, seg, B, out=hist)
        same = torch.equal(hist, torch_hist(bins, gh, rows, seg, B))
        nbytes = bins.numel() + gh.numel() * 4 + rows.numel() * 4
        src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        runs = {"kernel": lambda: device_ops.gbdt_histogram(bins, gh, rows, seg, B, out=hist),
                "torch": lambda: torch_hist(bins, gh, rows, seg, B),
                "copy": lambda: dst.copy_(src),
                "quantize": lambda: device_ops.gbdt_quantize(g, h, sg, sh, out=gh),
                "split": lambda: device_ops.gbdt_best_split(hist, sg, sh, 1.0),
                "multisplit": lambda: gbdt.gbdt_level_rows(node, slot_of_node, k)}
        times = {name: [] for name in runs}
        for name, fn in runs.items():      # warm up every shape the timed window uses
            fn()
        torch.cuda.synchronize()
        for _ in range(a.rounds):          # alternate, so drift hits every side alike
            for name, fn in runs.items():
                times[name] += timed(fn, 1 if name == "torch" else 5)
        med = {name: statistics.median(t) for name, t in times.items()}
        line = dict(n=n, F=F, B=B, k=k, bins=dist, same_bits=same, bytes=nbytes,
                    ms={name: round(v, 4) for name, v in med.items()},
                    ms_min_max={name: [round(min(t), 4), round(max(t), 4)] for name, t in times.items() if name in ("kernel", "torch")},
                    speedup=round(med["torch"] / med["kernel"], 2),
                    kernel_GBps=round(nbytes / med["kernel"] / 1e6, 1), copy_GBps=round(nbytes / med["copy"] / 1e6, 1),
                    hist_share_of_level=round(med["kernel"] / (med["kernel"] + med["split"] + med["multisplit"]), 3))
        lines.append(line)
        print(json.dumps(line), flush=True)
        del bins, gh, rows, src, dst, hist
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(x) for x in lines) + "\n")
    return 0 if all(x["same_bits"] for x in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
