#!/usr/bin/env python3
"""K18 on one process and one GPU: the forest walk kernel (``device_ops.gbdt_predict``) against a
vectorised torch form of the same definition (per tree ``steps`` rounds of ``gather`` over all rows, the sums
taken in tree order), alternating in one process.  There is no earlier GPU predictor to compare with.

The two results are compared bit for bit first, at the timed size.  Device-event times, one warm-up of every
arm, ``--rounds`` rounds; medians and min-max.  The bytes the algorithm needs (``n * F`` of bins, ``8 n`` of pred,
``8 n`` more with ``init``, ``4 n T`` with leaves; the forest is small beside them) over the kernel's call time
stand beside a plain copy of as many bytes timed in the same run.  ``--kernel-only`` runs each shape's kernel a
few times and nothing else: the run to put under a kernel trace, whose per-kernel times are the kernel
times.  One JSON line per shape.

Usage: python bench/gbdt_predict.py [--rounds 5] [--out FILE] [--quick] [--kernel-only]
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


def full_trees(T, depth, F, B, dev, gen):
    """T complete trees of ``depth`` levels below the root: random features and thresholds, random values."""
    size = 2 ** (depth + 1) - 1
    i = torch.arange(size, device=dev)
    inner = (2 * i + 2 < size)[None, :].expand(T, -1)
    feature = torch.randint(0, F, (T, size), device=dev, generator=gen)
    threshold = torch.randint(0, B - 1, (T, size), device=dev, generator=gen)
    left = (2 * i + 1)[None, :].expand(T, -1)
    minus = torch.full((T, size), -1, device=dev)
    nodes = torch.stack([torch.where(inner, feature, minus), torch.where(inner, threshold, minus),
                         torch.where(inner, left, minus), torch.where(inner, left + 1, minus)], dim=2)
    value = torch.randn(T * size, dtype=torch.float64, device=dev, generator=gen)
    off = (torch.arange(T + 1, device=dev) * size).to(torch.int32)
    return nodes.reshape(T * size, 4).to(torch.int32).contiguous(), value, off, size


def torch_form(bins, nodes, value, T, size, steps, init):
    """The definition on the GPU in plain torch: trees in order, ``steps`` rounds of gather a tree."""
    pred = torch.zeros(bins.shape[0], dtype=torch.float64, device=bins.device) if init is None else init.clone()
    nd = nodes.view(T, size, 4).to(torch.int64)
    for t in range(T):
        f, thr, left, right = nd[t].unbind(1)
        j = torch.zeros(bins.shape[0], dtype=torch.int64, device=bins.device)
        for _ in range(steps):
            fj = f[j]
            b = bins.gather(1, fj.clamp(min=0)[:, None])[:, 0].to(torch.int64)
            j = torch.where(fj >= 0, torch.where(b > thr[j], right[j], left[j]), j)
        pred = pred + value[t * size:(t + 1) * size][j]
    return pred


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="one small shape: a rehearsal of the script")
    ap.add_argument("--kernel-only", action="store_true", help="only the kernel, three calls a shape: for a kernel trace")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench/gbdt_predict.py measures on a GPU; none is visible")
    from mp4x.ops import device_ops
    dev = torch.device("cuda", 0)
    # (n, F, depth, T, init, leaves): r26's trainer shape, then a larger F whose bins are read from global memory
    shapes = [(1 << 14, 32, 6, 10, True, False)] if a.quick else \
        [(1 << 20, 32, 6, T, True, False) for T in (1, 100, 1000)] + [(1 << 20, 32, 6, 100, False, True),
                                                                     (1 << 20, 64, 6, 100, True, False)]
    B, lines = 64, []
    for n, F, depth, T, with_init, leaves in shapes:
        gen = torch.Generator(device=dev).manual_seed(n + F + T)
        bins = torch.randint(0, B, (n, F), dtype=torch.uint8, device=dev, generator=gen)
        nodes, value, off, size = full_trees(T, depth, F, B, dev, gen)
        init = torch.randn(n, dtype=torch.float64, device=dev, generator=gen) if with_init else None
        pred = torch.empty(n, dtype=torch.float64, device=dev)
        out = (pred, torch.empty(n, T, dtype=torch.int32, device=dev)) if leaves else pred

        def kernel():
            device_ops.gbdt_predict(bins, nodes, value, off, depth, init=init, leaves=leaves, out=out)

        if a.kernel_only:
            for _ in range(3):
                kernel()
            torch.cuda.synchronize()
            continue
        nbytes = n * F + 8 * n + (8 * n if with_init else 0) + (4 * n * T if leaves else 0)
        src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        kept = {}
        runs = {"kernel": kernel, "torch": lambda: kept.update(torch=torch_form(bins, nodes, value, T, size, depth, init)),
                "copy": lambda: dst.copy_(src)}
        for fn in runs.values():           # warm up every arm; the results of this pass are the ones compared
            fn()
        torch.cuda.synchronize()
        same = torch.equal(pred.view(torch.int64), kept["torch"].view(torch.int64))
        times = {name: [] for name in runs}
        for _ in range(a.rounds):          # alternate, so drift hits every arm alike
            for name, fn in runs.items():
                times[name] += timed(fn, 1 if name == "torch" and T > 100 else 3)
        med = {name: statistics.median(t) for name, t in times.items()}
        line = dict(n=n, F=F, depth=depth, T=T, init=with_init, leaves=leaves, same_bits=same, bytes=nbytes,
                    ms={name: round(v, 4) for name, v in med.items()},
                    ms_min_max={name: [round(min(t), 4), round(max(t), 4)] for name, t in times.items()},
                    kernel_vs_torch=round(med["torch"] / med["kernel"], 2),
                    kernel_GBps=round(nbytes / med["kernel"] / 1e6, 1), copy_GBps=round(nbytes / med["copy"] / 1e6, 1),
                    row_trees_per_us=round(n * T / med["kernel"] / 1e3, 1))
        lines.append(line)
        print(json.dumps(line), flush=True)
        del bins, src, dst, kept, out, pred
    if a.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(x) for x in lines) + "\n")
    return 0 if all(x["same_bits"] for x in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
