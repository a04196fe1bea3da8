#!/usr/bin/env python3
"""dispatchTokens + combineTokens three ways at one shape, p processes sharing GPU 0 (IPC kernels real,
no links between the ranks):

ragged   dispatchTokens(capacityFactor=f) -> combineTokens: the count exchange (a host sync) and shapes
         that follow the ids, every call
padded   dispatchTokens(sourceCapacity=S) -> combineTokens, eager: S = max(1, ceil(f * n / E)) with n
         this rank's assignments, so both forms offer every expert the same number of places in all
graph    the padded pair recorded once by comm.device.capture and replayed

Every call of a form is timed as the pair with device events on every rank; the forms alternate in
rounds and a row gives the slowest rank's median of the rounds' p50s with the rounds' extremes.  Then,
on rank 0 alone, the padded scatter + pad fill against the CLIP scatter with the quota keep[e] =
min(cnt[e], S) (the same kept rows; the padded form also writes the pad rows).
Default shape: bf16, 4096 tokens per rank x 7168, K = 8, 32 experts per rank, f = 1.0.
Prints one JSON line per row."""
import argparse
import json
import math
import multiprocessing as mp
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def worker(port, q, tokens, width, top_k, epr, iters, factor, rounds):
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
    S = max(1, math.ceil(factor * n / E))
    stats = comm.device.stats
    state = {}

    def ragged():
        rows, plan = comm.dispatchTokens(x, ids, E, capacityFactor=factor)
        state["ragged"] = comm.combineTokens(rows, plan, w)
        state["ragged_plan"] = plan

    def padded():
        rows, plan = comm.dispatchTokens(x, ids, E, sourceCapacity=S)
        state["padded"] = comm.combineTokens(rows, plan, w)
        state["padded_plan"] = plan

    for call in (ragged, padded):                      # warm both up; the large-message IPC instance appears here
        for _ in range(3):
            call()
    comm.barrier()
    graph = comm.device.capture(padded)
    forms = (("ragged", ragged), ("padded", padded), ("graph", graph.replay))
    p50s = {name: [] for name, _ in forms}
    ipc = {}
    for _ in range(rounds):                            # the forms alternate: a drifting clock hits all three
        for name, call in forms:
            comm.barrier()
            before = dict(stats)
            p50s[name].append(_p50(torch, call, iters, warm=1))
            moved = {k: v - before.get(k, 0) for k, v in stats.items() if v != before.get(k, 0)}
            ipc[name] = sum(v for k, v in moved.items() if k.startswith("all_to_all_v.ipc")) / (1 + iters)
    ipc["graph"] = 2.0                                 # recorded once: the replays launch what the capture saw
    out = []
    for name, _ in forms:
        v = sorted(p50s[name])
        out.append({"form": name, "p50_us": v[len(v) // 2], "min": v[0], "max": v[-1], "ipc_kernels_per_pair": ipc[name]})
    plan = state["padded_plan"]
    kept_padded, kept_ragged = int(plan.kept.sum()), sum(state["ragged_plan"].send_counts)
    kern = []
    comm.barrier()
    if r == 0:
        rb = width * 2
        flat = ids.reshape(-1).contiguous()
        rc = ops.moe_route_count(flat, E)
        keep = rc.counts[:E].clamp(max=S)
        kept = int(keep.sum())
        clip = torch.cat([keep, torch.cumsum(keep, 0) - keep]).contiguous()
        rows = torch.empty(kept, width, dtype=torch.bfloat16, device="cuda")
        buf = torch.empty(E * S, width, dtype=torch.bfloat16, device="cuda")
        s_clip = ops.moe_route_scatter(rc, x, top_k, rows, placed=kept, clip=clip)
        s_pad = ops.moe_route_scatter_pad(rc, x, top_k, buf, S)
        same = bool(torch.equal(s_clip >= 0, s_pad >= 0))
        for name, call, nbytes in (
                ("route_scatter_clip", lambda: ops.moe_route_scatter(rc, x, top_k, rows, placed=kept, clip=clip),
                 tokens * rb + kept * rb + n * 16 + 3 * 8 * n),
                ("route_scatter_pad + pad_fill", lambda: ops.moe_route_scatter_pad(rc, x, top_k, buf, S),
                 tokens * rb + E * S * rb + n * 16),
                ("pad_counts", lambda: ops.moe_pad_counts(rc, S), E * 16)):
            us = _p50(torch, call, iters)
            kern.append({"kernel": name, "p50_us": round(us, 1), "bytes": nbytes, "eff_gbps": round(nbytes / us / 1e3, 1),
                         "rows_kept": kept, "rows_written": kept if "clip" in name else E * S,
                         "same_assignments_kept": same})
    comm.barrier()
    comm.close(0)
    q.put((r, out, kern, S, kept_padded, kept_ragged))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=2)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tokens", type=int, default=4096, help="tokens per rank")
    ap.add_argument("--width", type=int, default=7168)
    ap.add_argument("--top-k", type=int, default=8)
    ap.add_argument("--experts-per-rank", type=int, default=32)
    ap.add_argument("--capacity-factor", type=float, default=1.0)
    a = ap.parse_args()
    os.environ.setdefault("MP4X_DEVICE_BACKEND", "gloo")
    os.environ.setdefault("MP4X_WATCHDOG", "0")
    os.environ.setdefault("MP4X_IPC_LARGE_BYTES", str(1 << 30))
    from mp4x import CommMaster
    m = CommMaster(a.procs, 0, host="127.0.0.1", exit_on_timeout=False, workdir=tempfile.mkdtemp()).start()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=worker, args=(m.port, q, a.tokens, a.width, a.top_k, a.experts_per_rank, a.iters,
                                              a.capacity_factor, a.rounds))
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
    E = a.experts_per_rank * a.procs
    shape = {"procs_on_one_gpu": a.procs, "dtype": "bfloat16", "tokens_per_rank": a.tokens, "width": a.width,
             "top_k": a.top_k, "experts": E, "capacity_factor": a.capacity_factor, "source_capacity": res[0][2],
             "padded_bytes_per_rank": E * res[0][2] * a.width * 2,
             "rows_kept_padded": [res[k][3] for k in sorted(res)], "rows_kept_ragged": [res[k][4] for k in sorted(res)]}
    for i, row in enumerate(res[0][0]):
        rows = [res[k][0][i] for k in sorted(res)]
        print(json.dumps({**shape, "form": row["form"], "phase": "dispatch + combine",
                          "ipc_kernels_per_pair": max(x["ipc_kernels_per_pair"] for x in rows),
                          "p50_us_median_of_rounds_max_rank": round(max(x["p50_us"] for x in rows), 1),
                          "min_of_rounds": round(min(x["min"] for x in rows), 1),
                          "max_of_rounds": round(max(x["max"] for x in rows), 1),
                          "links": "none: the ranks share one GPU"}), flush=True)
    for row in res[0][1]:
        print(json.dumps({**shape, **row, "measured_on": "rank 0 alone, the other ranks idle"}), flush=True)


if __name__ == "__main__":
    main()
