#!/usr/bin/env python3
"""Error feedback for the fp8 gradient reduce-scatter: what the residual costs.

kernel:  k_quant_ef against k_quant (csrc/kernels/codec.hip) on one tensor of --elements (64 Mi),
         f32 and bf16, hipEvents around each launch, the median of --iters after 3 warm-up
         launches, --rounds rounds with the two kernels alternating.  Bytes per element: k_quant
         reads es and writes 1 (+ 4 / 256 of scales); k_quant_ef also reads and writes 4 of residual.
         --lib PATH times k_quant of another build of libmp4x_hip.so in the same rounds (the parent
         commit's, to see that the existing kernel did not move).
rs:      IpcAllreduce.reduce_scatter_fp8 with and without a residual on one 16 MiB f32 tensor,
         --procs processes sharing GPU 0, p50 of --iters calls after 5 warm-up calls, the slowest
         rank, --rounds rounds with the two forms alternating.  Ranks that share one GPU have NO
         links between them (bench/fp8_rsag.py says what that means): the difference is the
         quantiser's extra HBM traffic on one device.

Prints one JSON line per measurement.
"""
import argparse
import ctypes
import json
import multiprocessing as mp
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median_ms(fn, iters):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(iters):
        s.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e))
    return sorted(ts)[len(ts) // 2]


def kernel(a):
    import torch
    from mp4x.operators import dtype_of_torch
    from mp4x.ops import device_ops as K
    torch.cuda.set_device(0)
    n = a.elements
    nblk = (n + 255) // 256
    other = None
    if a.lib:
        other = ctypes.CDLL(a.lib)
        other.mp4x_quant_fp8.restype = ctypes.c_int
        other.mp4x_quant_fp8.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_void_p]
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.randn(n, device="cuda").to(dtype)
        resid = torch.zeros(n, device="cuda")
        q = torch.empty(nblk * 256, dtype=torch.uint8, device="cuda")
        s = torch.empty(nblk, device="cuda")
        es = x.element_size()
        dt = int(dtype_of_torch(dtype))
        st = torch.cuda.current_stream().cuda_stream
        forms = [("k_quant", es + 1, lambda: K.quant_fp8(x, q, s)),
                 ("k_quant_ef", es + 9, lambda: K.quant_fp8_ef(x, resid, q, s))]
        if other is not None:
            def call_other():
                rc = other.mp4x_quant_fp8(dt, x.data_ptr(), n, q.data_ptr(), s.data_ptr(), st)
                assert rc == 0, rc
            forms.append(("k_quant (--lib)", es + 1, call_other))
        for rnd in range(a.rounds):
            for name, bpe, fn in forms:
                ms = _median_ms(fn, a.iters)
                nbytes = n * bpe + nblk * 4
                print(json.dumps({"bench": "kernel", "kernel": name, "dtype": str(dtype).replace("torch.", ""),
                                  "elements": n, "round": rnd, "bytes_per_element": bpe, "ms": round(ms, 4),
                                  "TBps": round(nbytes / ms / 1e9, 3)}), flush=True)


def rs_worker(port, q, n, iters, buf_bytes, rounds):
    import torch
    from mp4x import ProcessCommSlave
    from mp4x.parallel.ipc import IpcAllreduce
    from mp4x.utils.commutils import CommUtils
    torch.cuda.set_device(0)
    comm = ProcessCommSlave("b", "127.0.0.1", port, heartbeat=False)
    r, p = comm.getRank(), comm.getSlaveNum()
    ipc = IpcAllreduce(comm, nbytes=buf_bytes, slots=False)
    per = n // p // 64 * 64                                 # equal segments on the 16-byte grid
    froms, tos, _ = CommUtils.even_split(0, per * p, p)
    x0 = torch.randn(per * p, device="cuda", generator=torch.Generator(device="cuda").manual_seed(500 + r))
    x = x0.clone()
    resid = torch.zeros(per * p, device="cuda")
    forms = [("fp8", lambda: ipc.reduce_scatter_fp8(x, froms, tos)),
             ("fp8 + residual", lambda: ipc.reduce_scatter_fp8(x, froms, tos, residual=resid))]
    out = []
    for rnd, (form, call) in [(k, f) for k in range(rounds) for f in forms]:     # the two forms alternate
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
        ts = sorted(a_.elapsed_time(b_) for a_, b_ in zip(s, e))
        out.append({"form": form, "round": rnd, "ran": ok, "p50_us": ts[len(ts) // 2] * 1e3,
                    "p99_us": ts[min(len(ts) - 1, int(0.99 * len(ts)))] * 1e3, "err": ipc.error_word()})
        comm.barrier()
    ipc.close()
    comm.close(0)
    q.put((r, out))


def rs(a):
    from mp4x import CommMaster
    n = a.rs_elements
    m = CommMaster(a.procs, 0, host="127.0.0.1", exit_on_timeout=False, workdir=tempfile.mkdtemp()).start()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=rs_worker, args=(m.port, q, n, a.iters, a.buf_mib << 20, a.rounds)) for _ in range(a.procs)]
    for pr in ps:
        pr.start()
    res = dict(q.get(timeout=300) for _ in range(a.procs))
    for pr in ps:
        pr.join(timeout=30)
    m.stop(timeout=5)
    for i, row in enumerate(res[0]):
        rows = [res[k][i] for k in sorted(res)]
        print(json.dumps({"bench": "rs", "procs_on_one_gpu": a.procs, "dtype": "float32",
                          "range_bytes": n // a.procs // 64 * 64 * a.procs * 4, "form": row["form"], "round": row["round"],
                          "ran": all(x["ran"] for x in rows),
                          "p50_us_max_rank": round(max(x["p50_us"] for x in rows), 1),
                          "p99_us_max_rank": round(max(x["p99_us"] for x in rows), 1),
                          "err": max(x["err"] for x in rows), "links": "none: the ranks share one GPU"}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "rs"])
    ap.add_argument("--elements", type=int, default=64 << 20, help="kernel: elements of the tensor")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--lib", default=None, help="kernel: another libmp4x_hip.so whose k_quant is timed alongside")
    ap.add_argument("--procs", type=int, default=2)
    ap.add_argument("--rs-elements", type=int, default=4 << 20, help="rs: f32 elements (16 MiB)")
    ap.add_argument("--buf-mib", type=int, default=64)
    a = ap.parse_args()
    kernel(a) if a.what == "kernel" else rs(a)


if __name__ == "__main__":
    main()
