#!/usr/bin/env python3
"""K20 on one process and one GPU: the forest walk over float features (``device_ops.gbdt_predict_float``, one
launch, no bin tensor) against the two launches it replaces (``device_ops.gbdt_bin`` into a kept ``bins`` tensor,
then ``device_ops.gbdt_predict``), alternating in one process, and a plain device copy of as many bytes as the
one-launch path needs.

The shapes and forests are bench/gbdt_predict.py's (complete trees, B = 64), for float32 and bfloat16 features; one
value in 128 is NaN; the edges are ``gbdt_edges`` of the first 65536 rows and the float forest is ``float_forest`` of
the binned one.  The two paths' ``pred`` (and ``leaf``) are compared bit for bit first, at the timed size.
Device-event times, one warm-up of every arm, ``--rounds`` rounds of three calls; medians and min-max.  Bytes: ``e n
F`` of features (e = 4 or 2) for the one launch, ``(e + 2) n F`` for the two (the bins are written and read back),
plus ``8 n`` of pred, ``8 n`` of init and ``4 n T`` of leaves for either.  One JSON line per shape.

Usage: python bench/gbdt_predict_float.py [--rounds 5] [--out FILE] [--quick]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from gbdt_predict import full_trees, timed  # noqa: E402  (bench/gbdt_predict.py, next to this file)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="one small shape: a rehearsal of the script")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench/gbdt_predict_float.py measures on a GPU; none is visible")
    from mp4x.ops import device_ops
    from mp4x.parallel.gbdt import GbdtForest, float_forest, gbdt_edges
    dev = torch.device("cuda", 0)
    shapes = [(1 << 14, 32, 6, 10, True, False)] if a.quick else \
        [(1 << 20, 32, 6, T, True, False) for T in (1, 100, 1000)] + [(1 << 20, 32, 6, 100, False, True),
                                                                     (1 << 20, 64, 6, 100, True, False)]
    B, lines = 64, []
    for dtype in (torch.float32, torch.bfloat16):
        for n, F, depth, T, with_init, leaves in shapes:
            gen = torch.Generator(device=dev).manual_seed(n + F + T)
            X = torch.randn(n, F, device=dev, generator=gen)
            X[torch.rand(n, F, device=dev, generator=gen) < 1 / 128] = float("nan")
            X = X.to(dtype)
            edges, cnt = gbdt_edges(None, X[:65536], B)
            nodes, value, off, _ = full_trees(T, depth, F, B, dev, gen)
            fnodes = float_forest(GbdtForest(nodes, value, off, depth), edges, cnt).nodes
            init = torch.randn(n, dtype=torch.float64, device=dev, generator=gen) if with_init else None
            bins = torch.empty(n, F, dtype=torch.uint8, device=dev)
            outs = []
            for _ in range(2):
                pred = torch.empty(n, dtype=torch.float64, device=dev)
                outs.append((pred, torch.empty(n, T, dtype=torch.int32, device=dev)) if leaves else pred)

            def one_launch():
                device_ops.gbdt_predict_float(X, fnodes, value, off, depth, init=init, leaves=leaves, out=outs[0])

            def two_launches():
                device_ops.gbdt_bin(X, edges, cnt, 255, out=bins)
                device_ops.gbdt_predict(bins, nodes, value, off, depth, init=init, leaves=leaves, out=outs[1])

            e = X.element_size()
            rest = 8 * n + (8 * n if with_init else 0) + (4 * n * T if leaves else 0)
            nbytes = {"float": e * n * F + rest, "bin_walk": (e + 2) * n * F + rest}
            src = torch.empty(nbytes["float"], dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            runs = {"float": one_launch, "bin_walk": two_launches, "copy": lambda: dst.copy_(src)}
            for fn in runs.values():           # warm up every arm; the results of this pass are the ones compared
                fn()
            torch.cuda.synchronize()
            pair = (outs if leaves else [(o,) for o in outs])
            same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(*pair))
            times = {name: [] for name in runs}
            for _ in range(a.rounds):          # alternate, so drift hits every arm alike
                for name, fn in runs.items():
                    times[name] += timed(fn, 3)
            med = {name: statistics.median(t) for name, t in times.items()}
            line = dict(dtype=str(dtype).split(".")[1], n=n, F=F, depth=depth, T=T, init=with_init, leaves=leaves,
                        same_bits=same, bytes=nbytes, ms={name: round(v, 4) for name, v in med.items()},
                        ms_min_max={name: [round(min(t), 4), round(max(t), 4)] for name, t in times.items()},
                        bin_walk_vs_float=round(med["bin_walk"] / med["float"], 3),
                        float_GBps=round(nbytes["float"] / med["float"] / 1e6, 1),
                        bin_walk_GBps=round(nbytes["bin_walk"] / med["bin_walk"] / 1e6, 1),
                        copy_GBps=round(nbytes["float"] / med["copy"] / 1e6, 1))
            lines.append(line)
            print(json.dumps(line), flush=True)
            del X, bins, src, dst, outs, pred
    if a.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(x) for x in lines) + "\n")
    return 0 if all(x["same_bits"] for x in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
