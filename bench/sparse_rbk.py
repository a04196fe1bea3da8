#!/usr/bin/env python3
"""A/B of the sparse reduce-by-key (K5): the deterministic sort path (rocPRIM radix sort + run
starts + segmented reduce, csrc/kernels/sparse.hip) vs the hash path (K5h, open addressing +
row lists, csrc/kernels/sparse_hash.hip), its canonical form (K5c: priority insertion, a link pass,
an ordered compaction) and the dense path (K5d, direct addressing) on BASELINE
config 4's shape: the rows one owner receives at p ranks (200k keys x float[64] per rank, half
shared).  ``--dense-ids``: the keys are dictionary ids (the map API's numbering: the shared keys
0..99999, then every rank's own keys), so the sort runs over their bit width and K5d applies.
``--random-ids N``: one more data set of N rows keyed by random 64-bit ids (about a fifth of them
repeated).  The paths are timed in alternating rounds (``--rounds``: path A, path B, ..., path A,
...), so that drift of the shared machine hits them alike.  One JSON line per (data set, path):
p50 / min ms over all rounds' calls (hipEvents around each), the p50 of every round (their range is
the spread), exactness against the first path.
Run under rocprofv3 --kernel-trace --stats for the per-kernel split."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _config4(p, dim, dense_ids):
    import torch
    nkeys, shared = 200_000, 100_000
    ks, vs = [], []
    for r in range(p):
        own0 = shared + r * (nkeys - shared) if dense_ids else 10_000_000 + r * nkeys
        ids = torch.cat([torch.arange(shared), own0 + torch.arange(nkeys - shared)])
        ids = ids[ids % p == 0]
        ks.append(ids)
        vs.append(((ids.view(-1, 1) * 7 + torch.arange(dim) + r) % 23 - 11).float())
    return torch.cat(ks).cuda(), torch.cat(vs).cuda()


def _random_ids(n, dim):
    import torch
    g = torch.Generator().manual_seed(64)
    pool = torch.randint(-(1 << 62), 1 << 62, (n - n // 5,), generator=g) * 2 + 1
    keys = torch.cat([pool, pool[torch.randint(0, pool.numel(), (n // 5,), generator=g)]])
    keys = keys[torch.randperm(n, generator=g)]
    return keys.cuda(), torch.randint(-11, 12, (n, dim), generator=g).float().cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ps", default="2,8", help="config 4 at these rank counts ('' for none)")
    ap.add_argument("--iters", type=int, default=50, help="timed calls per path, over all rounds")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--paths", default="sort,hash", help="sort, hash, hashc, dense (with --dense-ids)")
    ap.add_argument("--dense-ids", action="store_true")
    ap.add_argument("--random-ids", type=int, default=0, metavar="N")
    args = ap.parse_args()
    import torch
    from mp4x.ops.device_ops import (dense_reduce_by_key, hash_reduce_by_key, hash_reduce_by_key_canonical,
                                     reduce_by_key)
    sets = [({"p": p}, p) + _config4(p, args.dim, args.dense_ids) for p in [int(x) for x in args.ps.split(",") if x]]
    if args.random_ids:
        sets.append(({"random_ids": args.random_ids}, 1) + _random_ids(args.random_ids, args.dim))
    paths = args.paths.split(",")
    per_round = max(1, args.iters // args.rounds)
    for tag, p, keys, rows in sets:
        bits = int(keys.max()).bit_length() if args.dense_ids else None
        base, T = int(keys.min()) // p, int(keys.max()) // p - int(keys.min()) // p + 1
        fns = {"sort": lambda: reduce_by_key(keys, rows, 0, key_bits=bits),
               "hash": lambda: hash_reduce_by_key(keys, rows, 0),
               "hashc": lambda: hash_reduce_by_key_canonical(keys, rows, 0),
               "dense": lambda: dense_reduce_by_key(keys, rows, 0, base, p, T)}
        res, ts, rp50 = {}, {x: [] for x in paths}, {x: [] for x in paths}
        for path in paths:
            for _ in range(5):
                res[path] = fns[path]()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for path in paths:
                cur = []
                for _ in range(per_round):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fns[path]()
                    b.record()
                    torch.cuda.synchronize()
                    cur.append(a.elapsed_time(b))
                ts[path] += cur
                rp50[path].append(round(sorted(cur)[len(cur) // 2], 4))
        for path in paths:
            t = sorted(ts[path])
            k, v, c = res[path]
            o = torch.argsort(k)
            res[path] = (k[o], v[o], c[o])
            print(json.dumps({**tag, "path": path, "rows": keys.numel(), "unique": int(k.numel()), "dim": args.dim,
                              "p50_ms": round(t[len(t) // 2], 4), "min_ms": round(t[0], 4), "round_p50_ms": rp50[path],
                              "row_bytes_in": keys.numel() * args.dim * 4}), flush=True)
        if len(res) >= 2:
            (k1, v1, c1), *rest = res.values()
            print(json.dumps({**tag, "exact": all(bool(torch.equal(k1, k2) and torch.equal(v1, v2) and
                                                       torch.equal(c1, c2)) for k2, v2, c2 in rest)}), flush=True)


if __name__ == "__main__":
    main()
