#!/usr/bin/env python3
"""Exact against fp8-coded reduce-scatter and all-gather on ONE tensor, p processes sharing GPU 0,
timed with hipEvents (p50 of --iters calls after 5 warm-up calls, slowest rank).

exact: IpcAllreduce.reduce_scatter / allgather (the staged direct forms);
fp8:   IpcAllreduce.reduce_scatter_fp8 / allgather_fp8 (K6 quantise + k_ipc_fp8_rs / k_ipc_fp8_ag).

Ranks that share one GPU have NO links between them: every "peer" read is a read of the same
HBM, so the codec's saving — a quarter of the f32 bytes per xGMI link — cannot show here, while
its cost (the quantise launch, the dequantise arithmetic) does.  The numbers say what the
protocol costs on one device, not what it gains over xGMI.  Prints one JSON line per (collective,
form).
"""
import argparse
import json
import multiprocessing as mp
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def worker(port, q, n, dtype_name, iters, buf_bytes):
    import torch
    from mp4x import Operators, ProcessCommSlave
    from mp4x.operators import dtype_of_torch, for_dtype
    from mp4x.parallel.ipc import IpcAllreduce
    from mp4x.utils.commutils import CommUtils
    torch.cuda.set_device(0)
    comm = ProcessCommSlave("b", "127.0.0.1", port, heartbeat=False)
    r, p = comm.getRank(), comm.getSlaveNum()
    dt = getattr(torch, dtype_name)
    ipc = IpcAllreduce(comm, nbytes=buf_bytes, slots=False)
    op = for_dtype(Operators.Float.SUM, dtype_of_torch(dt))
    per = n // p // 64 * 64                                 # equal segments on the 16-byte grid
    froms, tos, _ = CommUtils.even_split(0, per * p, p)
    x0 = torch.randn(per * p, device="cuda", generator=torch.Generator(device="cuda").manual_seed(500 + r)).to(dt)
    x = x0.clone()
    forms = [("reduce_scatter", "exact", lambda: ipc.reduce_scatter(x, froms, tos, op)),
             ("reduce_scatter", "fp8", lambda: ipc.reduce_scatter_fp8(x, froms, tos)),
             ("allgather", "exact", lambda: ipc.allgather(x, froms, tos)),
             ("allgather", "fp8", lambda: ipc.allgather_fp8(x, froms, tos))]
    out = []
    for coll, form, call in forms:
        x.copy_(x0)
        ok = True
        for _ in range(5):
            ok = bool(call()) and ok
        torch.cuda.synchronize()
        comm.barrier()
        s = [torch.cuda.Event(enable_timing=True) for _ in range(iters)]
        e = [torch.cuda.Event(enable_timing=True) for _ in range(iters)]
        for i in range(iters):
            x.copy_(x0)                                     # (outside the timed span: sums must not grow)
            s[i].record()
            call()
            e[i].record()
        torch.cuda.synchronize()
        ts = sorted(a.elapsed_time(b) for a, b in zip(s, e))
        out.append({"collective": coll, "form": form, "ran": ok, "p50_us": ts[len(ts) // 2] * 1e3,
                    "p99_us": ts[min(len(ts) - 1, int(0.99 * len(ts)))] * 1e3, "err": ipc.error_word()})
        comm.barrier()
    ipc.close()
    comm.close(0)
    q.put((r, out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=2)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--elements", type=int, default=4 << 20)
    ap.add_argument("--dtype", default="float32", choices=["float32", "bfloat16", "float16"])
    ap.add_argument("--buf-mib", type=int, default=64, help="IPC staging buffer; the exact forms need the whole range in it")
    a = ap.parse_args()
    from mp4x import CommMaster
    m = CommMaster(a.procs, 0, host="127.0.0.1", exit_on_timeout=False, workdir=tempfile.mkdtemp()).start()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=worker, args=(m.port, q, a.elements, a.dtype, a.iters, a.buf_mib << 20))
          for _ in range(a.procs)]
    for pr in ps:
        pr.start()
    res = dict(q.get(timeout=300) for _ in range(a.procs))
    for pr in ps:
        pr.join(timeout=30)
    m.stop(timeout=5)
    es = 4 if a.dtype == "float32" else 2
    for i, row in enumerate(res[0]):
        rows = [res[k][i] for k in sorted(res)]
        print(json.dumps({"procs_on_one_gpu": a.procs, "dtype": a.dtype, "range_bytes": a.elements // a.procs // 64 * 64 * a.procs * es,
                          "collective": row["collective"], "form": row["form"], "ran": all(x["ran"] for x in rows),
                          "p50_us_max_rank": round(max(x["p50_us"] for x in rows), 1),
                          "p99_us_max_rank": round(max(x["p99_us"] for x in rows), 1),
                          "err": max(x["err"] for x in rows), "links": "none: the ranks share one GPU"}))


if __name__ == "__main__":
    main()
