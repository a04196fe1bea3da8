#!/usr/bin/env python3
"""Exact against fp8-coded alltoallArray on ONE send tensor per rank, p processes sharing GPU 0,
timed with hipEvents (p50 of --iters calls after 5 warm-up calls, slowest rank).

exact: comm.alltoallArray(send, counts) — the IPC copy-plan kernel moving full-width rows;
fp8:   comm.alltoallArray(send, counts, operand=...(codec="fp8")) — K6 quantise + k_ipc_fp8_a2a.

Both forms include the count-matrix exchange every call makes.  Default shape: bf16, 4096 rows of
7168 per rank, even counts (expert-parallel token dispatch).

Ranks that share one GPU have NO links between them: every "peer" read is a read of the same
HBM, so the codec's saving — half of the bf16 bytes per xGMI link — cannot show here, while its
cost (the quantise launch, the dequantise arithmetic) does.  The numbers say what the protocol
costs on one device, not what it gains over xGMI.  Prints one JSON line per form.
"""
import argparse
import json
import multiprocessing as mp
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP8, IPC = "all_to_all_v.fp8.ipc", "all_to_all_v.ipc"


def worker(port, q, rows, width, dtype_name, iters):
    import torch
    from mp4x import Operands, ProcessCommSlave
    torch.cuda.set_device(0)
    os.environ.setdefault("MP4X_DEVICE_INDEX", "0")
    comm = ProcessCommSlave("b", "127.0.0.1", port, heartbeat=False)
    r, p = comm.getRank(), comm.getSlaveNum()
    dt = getattr(torch, dtype_name)
    make = {"float32": Operands.FLOAT_OPERAND, "bfloat16": Operands.BF16_OPERAND, "float16": Operands.HALF_OPERAND}
    operand = make[dtype_name](codec="fp8")
    counts = [rows // p] * p
    send = torch.randn(sum(counts), width, device="cuda",
                       generator=torch.Generator(device="cuda").manual_seed(700 + r)).to(dt)
    recv = torch.empty_like(send)
    stats = comm.device.stats
    forms = [("exact", IPC, lambda: comm.alltoallArray(send, counts, recv)),
             ("fp8", FP8, lambda: comm.alltoallArray(send, counts, recv, operand))]
    out = []
    for form, counter, call in forms:
        before = stats.get(counter, 0)
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        comm.barrier()
        s = [torch.cuda.Event(enable_timing=True) for _ in range(iters)]
        e = [torch.cuda.Event(enable_timing=True) for _ in range(iters)]
        for i in range(iters):
            s[i].record()
            call()
            e[i].record()
        torch.cuda.synchronize()
        ts = sorted(a.elapsed_time(b) for a, b in zip(s, e))
        out.append({"form": form, "ran": stats.get(counter, 0) - before == 5 + iters,
                    "p50_us": ts[len(ts) // 2] * 1e3, "p99_us": ts[min(len(ts) - 1, int(0.99 * len(ts)))] * 1e3})
        comm.barrier()
    comm.close(0)
    q.put((r, out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=2)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rows", type=int, default=4096, help="rows each rank sends, split evenly over the ranks")
    ap.add_argument("--width", type=int, default=7168)
    ap.add_argument("--dtype", default="bfloat16", choices=["float32", "bfloat16", "float16"])
    a = ap.parse_args()
    os.environ.setdefault("MP4X_DEVICE_BACKEND", "gloo")
    from mp4x import CommMaster
    m = CommMaster(a.procs, 0, host="127.0.0.1", exit_on_timeout=False, workdir=tempfile.mkdtemp()).start()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=worker, args=(m.port, q, a.rows, a.width, a.dtype, a.iters)) for _ in range(a.procs)]
    for pr in ps:
        pr.start()
    res = dict(q.get(timeout=300) for _ in range(a.procs))
    for pr in ps:
        pr.join(timeout=30)
    m.stop(timeout=5)
    es = 4 if a.dtype == "float32" else 2
    for i, row in enumerate(res[0]):
        rows = [res[k][i] for k in sorted(res)]
        print(json.dumps({"procs_on_one_gpu": a.procs, "dtype": a.dtype, "rows_per_rank": a.rows // a.procs * a.procs,
                          "width": a.width, "send_bytes_per_rank": a.rows // a.procs * a.procs * a.width * es,
                          "form": row["form"], "ran": all(x["ran"] for x in rows),
                          "p50_us_max_rank": round(max(x["p50_us"] for x in rows), 1),
                          "p99_us_max_rank": round(max(x["p99_us"] for x in rows), 1),
                          "links": "none: the ranks share one GPU"}), flush=True)


if __name__ == "__main__":
    main()
