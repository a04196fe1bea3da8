#!/usr/bin/env python3
"""Expert-parallel token dispatch / combine: the new calls against the torch composition a caller
writes on alltoallArray alone, p processes sharing GPU 0, timed with hipEvents (p50 of --iters calls
after 3 warm-up calls, slowest rank).  Default shape: bf16, 4096 tokens x 7168 per rank, K = 8 distinct
experts per token (top-k of random logits), E = 32 * p.

new:    rows, plan = comm.dispatchTokens(x, ids, E);  out = comm.combineTokens(rows, plan, w)
torch:  dispatch = argsort(ids) + index_select + bincount + alltoallArray of the rows AND of the ids
        (the receiver needs them to regroup) + argsort + index_select;
        combine  = index_copy back to source order + alltoallArray + index_add_ (f32 atomics) + cast.

It also times the three K9 kernels alone on rank 0 (the other ranks wait at a barrier) and gives
their effective GB/s — bytes the algorithm must move over the p50 — next to the K1 copy ceiling on
record (profiles/r6/n1/kernel_stats.csv: 1 GB copied in 331 us, 6.0 TB/s read + write).

Ranks that share one GPU have NO links between them: every "peer" read of the all-to-all is a read of
the same HBM, and the ranks' kernels share its bandwidth.  The numbers say what the routing costs
around the transport on one device; nothing here has been measured over real xGMI.  The send buffer
of the default shape (470 MB) needs MP4X_IPC_LARGE_BYTES = 512 MiB, which this script sets.

--capacity-factor F: dispatchTokens(capacityFactor=F).  The torch composition has no capacity, so it
is not timed then and the two forms' results are not compared; the kernel rows gain the clipped
route scatter along the plan's quota (bytes: the rows it keeps) next to the unclipped one.
Prints one JSON line per row.
"""
import argparse
import json
import multiprocessing as mp
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IPC = "all_to_all_v.ipc"
K1_COPY_TBPS = 6.0


def _p50(torch, call, iters, warm=3):
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    s = [torch.cuda.Event(enable_timing=True) for _ in range(iters)]
    e = [torch.cuda.Event(enable_timing=True) for _ in range(iters)]
    for i in range(iters):
        s[i].record()
        call()
        e[i].record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in zip(s, e))
    return ts[len(ts) // 2] * 1e3


def worker(port, q, tokens, width, top_k, epr, iters, capacity_factor=None):
    import torch
    from mp4x import ProcessCommSlave
    from mp4x.ops import device_ops as ops
    torch.cuda.set_device(0)
    os.environ.setdefault("MP4X_DEVICE_INDEX", "0")
    comm = ProcessCommSlave("b", "127.0.0.1", port, heartbeat=False)
    r, p = comm.getRank(), comm.getSlaveNum()
    E = epr * p
    g = torch.Generator(device="cuda").manual_seed(900 + r)
    x = torch.randn(tokens, width, device="cuda", generator=g).to(torch.bfloat16)
    logits = torch.randn(tokens, E, device="cuda", generator=g)
    w, ids = torch.topk(torch.softmax(logits, -1), top_k, dim=-1)
    w = w.contiguous()
    n = tokens * top_k
    stats = comm.device.stats
    state = {}

    def new_dispatch():
        state["rows"], state["plan"] = comm.dispatchTokens(x, ids, E, capacityFactor=capacity_factor)

    def new_combine():
        state["out"] = comm.combineTokens(state["rows"], state["plan"], w)

    def torch_dispatch():
        flat = ids.reshape(-1)
        order = torch.argsort(flat, stable=True)
        sorted_ids = flat[order]
        send = x.index_select(0, order // top_k)
        counts = torch.bincount(sorted_ids // epr, minlength=p).tolist()
        recv, rc = comm.alltoallArray(send, counts)
        rid, _ = comm.alltoallArray(torch.stack([sorted_ids, sorted_ids], 1), counts)    # 16-byte rows
        order2 = torch.argsort(rid[:, 0], stable=True)
        state.update(t_rows=recv.index_select(0, order2), order=order, order2=order2, rc=rc,
                     expert_counts=torch.bincount(rid[:, 0] - r * epr, minlength=epr))

    def torch_combine():
        y = state["t_rows"]
        src = torch.empty_like(y)
        src.index_copy_(0, state["order2"], y)
        back, _ = comm.alltoallArray(src, state["rc"])
        order = state["order"]
        acc = torch.zeros(tokens, width, dtype=torch.float32, device="cuda")
        acc.index_add_(0, order // top_k, back.to(torch.float32) * w.reshape(-1)[order].unsqueeze(1))
        state["t_out"] = acc.to(torch.bfloat16)

    out = []
    for form, phase, call, a2a in [("new", "dispatch", new_dispatch, 1), ("torch", "dispatch", torch_dispatch, 2),
                                   ("new", "combine", new_combine, 1), ("torch", "combine", torch_combine, 1)]:
        if form == "torch" and capacity_factor is not None:
            continue
        comm.barrier()
        before = stats.get(IPC, 0)
        us = _p50(torch, call, iters)
        out.append({"form": form, "phase": phase, "p50_us": us, "ipc": stats.get(IPC, 0) - before == a2a * (3 + iters)})
    # the same rows on both paths (the experts' groups in the same order; the combine's sums differ in
    # the last bits only: index_add_ takes the K terms in any order)
    same_rows = close = None
    if capacity_factor is None:
        same_rows = bool(torch.equal(state["rows"], state["t_rows"]))
        close = bool(torch.allclose(state["out"].float(), state["t_out"].float(), rtol=2e-2, atol=2e-2))
    kern = []
    comm.barrier()
    if r == 0:
        rb = width * 2
        flat = ids.reshape(-1).contiguous()
        rc = ops.moe_route_count(flat, E)
        rows = torch.empty(n, width, dtype=torch.bfloat16, device="cuda")
        slots = ops.moe_route_scatter(rc, x, top_k, rows)
        calls = [("route_count", lambda: ops.moe_route_count(flat, E), n * 8),
                 ("route_scatter", lambda: ops.moe_route_scatter(rc, x, top_k, rows, placed=n),
                  tokens * rb + n * rb + n * 16),
                 ("combine", lambda: ops.moe_combine(rows, slots, w, tokens, top_k, max_slot=n - 1),
                  n * rb + tokens * rb + n * 12)]
        if capacity_factor is not None:
            # the plan's quota of this rank: every token row is still read (at least one of its K
            # assignments almost surely stays), only the kept rows are written; the three 8-byte
            # table gathers per assignment are counted at face value though they hit the L2
            plan = state["plan"]
            kept = sum(plan.send_counts)
            calls.insert(2, ("route_scatter_clip",
                             lambda: ops.moe_route_scatter(rc, x, top_k, rows, placed=kept, clip=plan._clip),
                             tokens * rb + kept * rb + n * 16 + 3 * 8 * n))
        for name, call, nbytes in calls:
            us = _p50(torch, call, iters)
            kern.append({"kernel": name, "p50_us": round(us, 1), "bytes": nbytes, "eff_gbps": round(nbytes / us / 1e3, 1),
                         "k1_copy_ceiling_gbps": K1_COPY_TBPS * 1e3})
    comm.barrier()
    comm.close(0)
    q.put((r, out, same_rows, close, kern))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=2)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--tokens", type=int, default=4096, help="tokens per rank")
    ap.add_argument("--width", type=int, default=7168)
    ap.add_argument("--top-k", type=int, default=8)
    ap.add_argument("--experts-per-rank", type=int, default=32)
    ap.add_argument("--capacity-factor", type=float, default=None,
                    help="dispatchTokens(capacityFactor=): every expert accepts max(1, ceil(f * N / E)) assignments")
    a = ap.parse_args()
    os.environ.setdefault("MP4X_DEVICE_BACKEND", "gloo")
    os.environ.setdefault("MP4X_IPC_LARGE_BYTES", str(512 << 20))
    from mp4x import CommMaster
    m = CommMaster(a.procs, 0, host="127.0.0.1", exit_on_timeout=False, workdir=tempfile.mkdtemp()).start()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=worker, args=(m.port, q, a.tokens, a.width, a.top_k, a.experts_per_rank, a.iters,
                                              a.capacity_factor))
          for _ in range(a.procs)]
    for pr in ps:
        pr.start()
    res = {}
    for _ in range(a.procs):
        got = q.get(timeout=600)
        res[got[0]] = got[1:]
    for pr in ps:
        pr.join(timeout=30)
    m.stop(timeout=5)
    shape = {"procs_on_one_gpu": a.procs, "dtype": "bfloat16", "tokens_per_rank": a.tokens, "width": a.width,
             "top_k": a.top_k, "experts": a.experts_per_rank * a.procs, "capacity_factor": a.capacity_factor,
             "routed_bytes_per_rank": a.tokens * a.top_k * a.width * 2}
    for i, row in enumerate(res[0][0]):
        rows = [res[k][0][i] for k in sorted(res)]
        print(json.dumps({**shape, "form": row["form"], "phase": row["phase"],
                          "one_ipc_all_to_all_per_call": all(x["ipc"] for x in rows),
                          "p50_us_max_rank": round(max(x["p50_us"] for x in rows), 1),
                          "links": "none: the ranks share one GPU"}), flush=True)
    if a.capacity_factor is None:
        print(json.dumps({**shape, "same_rows_both_forms": all(res[k][1] for k in res),
                          "combine_close_both_forms": all(res[k][2] for k in res)}), flush=True)
    for row in res[0][3]:
        print(json.dumps({**shape, **row, "measured_on": "rank 0 alone, the other ranks idle"}), flush=True)


if __name__ == "__main__":
    main()
