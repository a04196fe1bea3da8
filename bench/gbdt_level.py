#!/usr/bin/env python3
"""K17 A/B on one process and one GPU: one level advance of the fixed-point GBDT from k parents to 2k
children, three ways, alternating in one process:

  sort       the default level: ``gbdt_level_rows`` (torch stable sort of all rows by node) + a histogram
             of the 2k children
  partition  ``device_ops.gbdt_partition`` + a histogram of the 2k children
  subtract   ``device_ops.gbdt_partition`` + a histogram of the k first (smaller) children +
             ``device_ops.gbdt_hist_subtract`` against the kept parent histograms

The three results (rows, table, histograms) are compared bit for bit first.  Device-event times, one
warm-up of every arm, ``--rounds`` rounds; medians and min-max.  The partition alone is reported with its
bytes (``12 m`` of row slots and masks + ``m`` gathered bytes) over its time, beside a plain copy of as many
bytes in the same run.  Nothing here runs two ranks on one GPU or more than one GPU.  One JSON line per
shape.

Usage: python bench/gbdt_level.py [--rounds 5] [--out FILE] [--quick]
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
        raise SystemExit("bench/gbdt_level.py measures on a GPU; none is visible")
    from mp4x.ops import device_ops
    from mp4x.parallel import gbdt
    dev = torch.device("cuda", 0)
    shapes = [(1 << 16, 28, 8)] if a.quick else [(n, F, k) for n in (1 << 20, 1 << 23) for F in (28, 128) for k in (1, 8, 32)]
    B, lines = 256, []
    for n, F, k in shapes:
        gen = torch.Generator(device=dev).manual_seed(n + F + k)
        bins = torch.randint(0, B, (n, F), dtype=torch.uint8, device=dev, generator=gen)
        gh = torch.randint(-2 ** 30, 2 ** 30, (n, 2), dtype=torch.int32, device=dev, generator=gen)
        node = torch.randint(0, k, (n,), device=dev, generator=gen)
        rows, seg = gbdt.gbdt_level_rows(node, torch.arange(k, device=dev), k)
        feature = torch.randint(0, F, (k,), device=dev, generator=gen)
        threshold = torch.randint(0, B - 1, (k,), device=dev, generator=gen)
        right = bins.gather(1, feature[node][:, None])[:, 0].to(torch.int64) > threshold[node]
        n_right = torch.bincount(node[right], minlength=k)
        first_right = (2 * n_right < torch.bincount(node, minlength=k)).to(torch.int64)      # the smaller child first
        # the default's move: child 2j + went_right; slot j the first child of j, slot k + j the second
        node2 = 2 * node + right.to(torch.int64)
        slot_of_node = torch.empty(2 * k, dtype=torch.int64, device=dev)
        slot_of_node[2 * torch.arange(k, device=dev) + first_right] = torch.arange(k, device=dev)
        slot_of_node[2 * torch.arange(k, device=dev) + 1 - first_right] = k + torch.arange(k, device=dev)
        f32, t32, r32 = (t.to(torch.int32) for t in (feature, threshold, first_right))
        parent = device_ops.gbdt_histogram(bins, gh, rows, seg, B)
        parent_of = torch.arange(k, dtype=torch.int32, device=dev)
        rows2, seg2 = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(2 * k + 1, dtype=torch.int64, device=dev)
        hists = {name: torch.empty(2 * k, F, B, 2, dtype=torch.int64, device=dev) for name in ("sort", "partition", "subtract")}
        kept = {}

        def sort_arm():
            kept["sort"] = gbdt.gbdt_level_rows(node2, slot_of_node, 2 * k)
            device_ops.gbdt_histogram(bins, gh, *kept["sort"], B, out=hists["sort"])

        def part():
            device_ops.gbdt_partition(bins, rows, seg, f32, t32, r32, out=(rows2, seg2))

        def partition_arm():
            part()
            device_ops.gbdt_histogram(bins, gh, rows2, seg2, B, out=hists["partition"])

        def subtract_arm():
            part()
            device_ops.gbdt_histogram(bins, gh, rows2, seg2[:k + 1], B, out=hists["subtract"][:k])
            device_ops.gbdt_hist_subtract(parent, hists["subtract"][:k], parent_of, out=hists["subtract"][k:])

        nbytes = 13 * n
        src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        runs = {"sort": sort_arm, "partition": partition_arm, "subtract": subtract_arm, "partition_only": part,
                "sort_only": lambda: gbdt.gbdt_level_rows(node2, slot_of_node, 2 * k), "copy": lambda: dst.copy_(src)}
        for fn in runs.values():           # warm up every arm; the results of this pass are the ones compared
            fn()
        torch.cuda.synchronize()
        same = torch.equal(rows2, kept["sort"][0]) and torch.equal(seg2, kept["sort"][1]) and \
            torch.equal(hists["partition"], hists["sort"]) and torch.equal(hists["subtract"], hists["sort"])
        times = {name: [] for name in runs}
        for _ in range(a.rounds):          # alternate, so drift hits every arm alike
            for name, fn in runs.items():
                times[name] += timed(fn, 3)
        med = {name: statistics.median(t) for name, t in times.items()}
        line = dict(n=n, F=F, B=B, k=k, same_bits=same, first_child_rows=int(seg2[k]), bytes=nbytes,
                    ms={name: round(v, 4) for name, v in med.items()},
                    ms_min_max={name: [round(min(t), 4), round(max(t), 4)] for name, t in times.items()},
                    partition_vs_sort=round(med["sort"] / med["partition"], 2),
                    subtract_vs_sort=round(med["sort"] / med["subtract"], 2),
                    partition_GBps=round(nbytes / med["partition_only"] / 1e6, 1),
                    copy_GBps=round(nbytes / med["copy"] / 1e6, 1))
        lines.append(line)
        print(json.dumps(line), flush=True)
        del bins, gh, rows, rows2, src, dst, hists, parent, kept
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(x) for x in lines) + "\n")
    return 0 if all(x["same_bits"] for x in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
