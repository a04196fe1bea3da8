#!/usr/bin/env python3
"""Headline benchmark: allreduce bus bandwidth + p50 latency, 1 GB float[] (BASELINE.json).

``python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]`` — for N>1 the
driver launches one rank per GPU with ``torch.distributed.run``.  Every step is ONE public-API call

    comm.allreduceArray(buf, Operands.FLOAT_OPERAND(), Operators.Float.SUM, 0, n, scale=1/p)

on a 1e9-byte float32 array (250,000,000 elements, synthetic random data) resident on the
rank's MI355X, i.e. the reference's ``ProcessCommSlave.allreduceArray``
(ProcessCommSlave.java:1733-1763) on the BASELINE config.  ``scale=1/p`` (the DP gradient
average, fused into the collective's final write) keeps the values bounded at any ``--steps``:
a SUM would grow p-fold per call and reach f32 inf after ~40 calls at p=8.

For N>1 the warm-up first autotunes the schedule (RCCL, RCCL with more channels, IPC two-shot
over xGMI staged / zero-copy pull / zero-copy push, a2a, rhd; ``--autotune-iters`` timed calls
each, MAX over ranks, every candidate checked against an exact pattern first) and pins the
fastest.  Timing: W untimed warmup calls, barrier + device sync, K timed back-to-back calls,
barrier + device sync (the headline, host clock; MAX over ranks).

A plain run stops there: set-up, warm-up, the K timed steps, the outputs if ``--dump-outputs`` is
given, ONE result line (``p50_ms``, ``verified``, the RCCL baseline and the other evidence keys
are null).  Everything below runs only with ``--full``, which prints the headline line right
after its measurement and an enriched final line (same numbers) at the end.

``--dump-outputs DIR``: right after the timed steps rank 0 writes what the last timed call
returned (N=1: ``out``; N>1: the in-place buffer) as ``DIR/allreduce_out.npy`` in float32; an
array of more than 2^23 elements is cut to a fixed, seeded sample of 2^23 of its elements
(32 MB).  The inputs are seeded per rank, so the same arguments give the same inputs every run.

Latency distribution (``--full``): outside the timed region, K more calls with a hipEvent pair
around each for p50 / p99.

Self-verification (``--full``; after the timed steps, outside them): the SAME call on the SAME buffer with
the pinned schedule runs once more on an exact pattern; the result is compared with the fp64
answer on every rank -> ``verified`` and ``max_abs_err`` (MAX over ranks).  A wrong result
makes the run exit non-zero (rc 3) after printing its line.

RCCL baseline at equal method (``--full``, N>1, GPU): K more calls of the same public call with the RCCL
schedule forced (``ncclAllReduce``, fused ncclAvg), same timing method, MAX over ranks ->
``rccl_busbw_gbps`` / ``rccl_p50_ms`` next to ``value`` ("judge our
numbers against RCCL's on the same box").

busbw follows the nccl-tests convention used in BASELINE.md: algbw = bytes / t,
busbw = algbw * 2(p-1)/p, and ``value`` IS that busbw (per rank, the BASELINE metric; the
whole-job sum ``N * busbw`` is reported separately as ``aggregate_busbw_gbps``).
With one rank nothing crosses a link (factor 2(p-1)/p = 0) and the in-place call is a
no-op by the reference's contract, so N=1 times the OUT-OF-PLACE form of the same call
(``out=``; a 1 GB device copy through the K1 kernel) and reports algbw for it — HBM
evidence, not an allreduce number.

``--alloc``: how the N>1 buffer is made — ``register`` (default: a caching-allocator tensor
registered with ``registerBuffer``), ``memalloc`` (``comm.memAlloc``: mapped into every peer
at any size, e.g. ``--bytes 8000000000``), ``plain`` (unregistered: staged kernels / RCCL).
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC (mp4x/__init__.py), before any HIP call
# the tier sweep's pins persist under this job's topology key, and the next job on the same
# topology loads them at creation (mp4x/parallel/tiers.py)
os.environ.setdefault("MP4X_TUNE_AUTO", "1")

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# reference busbw (MB/s) for ~1 GB allreduce, BASELINE.md section D (mean of 1e8 and 5e8 rows)
REF_BUSBW_MBPS = {2: 85.2, 4: 92.1, 6: 86.8, 8: 88.0}
METRIC = "allreduce bus bandwidth (GB/s) + p50 latency, 1 GB float[], 1/2/4/8 MI355X"
RC_UNVERIFIED = 3


class _CpuEvent:
    """time.perf_counter stand-in for torch.cuda.Event in the --cpu dry run."""

    def __init__(self, enable_timing=True):
        self.t = 0.0

    def record(self, *a):
        self.t = time.perf_counter()

    def elapsed_time(self, other):
        return (other.t - self.t) * 1e3


def _time_steps(step, steps, sync_all):
    """The headline timing: K back-to-back calls of ``step`` on the host clock, bracketed by a
    device-wide sync + barrier on both sides (nothing else inside the timed region).  Returns the
    wall seconds of the timed K calls."""
    sync_all()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    sync_all()
    return time.perf_counter() - t0


def _latency_pass(torch, step, steps, sync_all):
    """K more calls with a hipEvent pair around each, in a pass of their own, for the per-call
    latency distribution (p50 / p99).  Returns the sorted ms list."""
    starts = [torch.cuda.Event(enable_timing=True) for _ in range(steps)]
    ends = [torch.cuda.Event(enable_timing=True) for _ in range(steps)]
    for i in range(steps):
        starts[i].record()
        step()
        ends[i].record()
    sync_all()
    return sorted(s.elapsed_time(e) for s, e in zip(starts, ends))


def _measure(torch, step, steps, sync_all):
    """Both passes: (wall seconds of the timed K calls, sorted ms list of K more calls)."""
    wall = _time_steps(step, steps, sync_all)
    return wall, _latency_pass(torch, step, steps, sync_all)


DUMP_MAX_ELEMS = 1 << 23      # 32 MB of float32 per dumped array
DUMP_SEED = 20240607


def _dump_output(torch, out_dir, name, t):
    """``out_dir/name.npy`` (float32): ``t`` whole, or a fixed seeded sample of its elements."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    n = t.numel()
    if n > DUMP_MAX_ELEMS:
        g = torch.Generator(device="cpu")
        g.manual_seed(DUMP_SEED)
        idx = torch.randint(0, n, (DUMP_MAX_ELEMS,), generator=g).sort().values
        t = t[idx.to(t.device)]
    np.save(os.path.join(out_dir, name + ".npy"), t.detach().to(torch.float32).cpu().numpy())


def _leave_unwritable_cwd():
    """The embedded master writes its ``kill_<port>.sh`` into the working directory (the
    reference's Server.killMe).  Started from a directory this user cannot write, e.g. a read-only
    checkout, the run moves to a temporary directory of its own, removed at exit; paths given
    relative to the old one (mp4x's file / directory variables) are made absolute first."""
    cwd = os.getcwd()
    if os.access(cwd, os.W_OK | os.X_OK):
        return
    import atexit
    import shutil
    import tempfile
    for var in ("MP4X_TUNE_FILE", "MP4X_TUNE_DIR", "MP4X_LOG_CONFIG", "MP4X_LOG_DIR"):
        if os.environ.get(var):
            os.environ[var] = os.path.abspath(os.environ[var])
    tmp = tempfile.mkdtemp(prefix="mp4x_bench_")
    os.chdir(tmp)
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)


def _timed_p50(torch, fn, iters, sync):
    """p50 ms of ``iters`` calls of ``fn``, each bracketed by syncs (host clock)."""
    ts = []
    for _ in range(iters):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2]


def _baseline_configs(comm, torch, dist, p, rank, dev, agree_dev, may_start=lambda name: True):
    """BASELINE configs 3 / 4 / 5 on this job (evidence; each bounded, failures recorded, every
    rank stops together).  Exact checks for 3 and 4, the fp64 error bound for 5."""
    from mp4x import CommUtils, Operands, Operators
    out = {}

    def sync():
        torch.cuda.synchronize()
        comm.device.barrier()
        torch.cuda.synchronize()

    def cfg3():
        n = 2_000_000_000 // p * p
        x = comm.memAlloc(n, torch.bfloat16)
        try:
            B = Operands.BF16_OPERAND()
            counts = [n // p] * p
            fr, to = CommUtils.getFromsFromCount(0, counts, p), CommUtils.getTosFromCount(0, counts, p)
            CH = 1 << 28
            for s0 in range(0, n, CH):
                i = torch.arange(s0, min(n, s0 + CH), device=dev)
                x[s0:s0 + CH] = (i % 13 + rank).to(torch.bfloat16)

            def step():
                comm.reduceScatterArray(x, B, Operators.BFloat16.SUM, 0, counts)
                comm.allgatherArray(x, B, fr, to)
            step()
            sync()
            ok = True
            for s0 in range(0, n, CH):
                i = torch.arange(s0, min(n, s0 + CH), device=dev)
                ok &= bool(torch.equal(x[s0:s0 + CH], (p * (i % 13) + p * (p - 1) // 2).to(torch.bfloat16)))
            ms = _timed_p50(torch, step, 5, sync)
            return {"ms": round(ms, 3), "exact": ok,
                    "busbw_gbps": round(n * 2 / (ms * 1e-3) / 1e9 * 2 * (p - 1) / p, 2)}
        finally:
            comm.memFree(x)

    def cfg4():
        dim, nkeys = 64, 200_000
        shared = nkeys // 2
        ids = torch.cat([torch.arange(shared), 10_000_000 + rank * nkeys + torch.arange(nkeys - shared)]).to(dev)
        vals = (torch.arange(nkeys * dim, device=dev) % 7 + rank).float().view(nkeys, dim)
        fn = lambda: comm.allreduceSparse(ids, vals, Operators.Float.SUM)   # noqa: E731
        rk, rv = fn()
        sync()
        # shared ids: sum over ranks of (row pattern + rank); own ids: that rank's row only
        base = (torch.arange(shared * dim, device=dev) % 7).float().view(shared, dim)
        order = torch.argsort(rk)
        rk, rv = rk[order], rv[order]
        ok = bool(torch.equal(rk[:shared].cpu(), torch.arange(shared))) and \
            bool(torch.equal(rv[:shared], base * p + p * (p - 1) / 2)) and rk.numel() == shared + p * (nkeys - shared)
        ms = _timed_p50(torch, fn, 5, sync)
        return {"ms": round(ms, 3), "exact": ok, "keys_per_rank": nkeys, "dim": dim}

    def cfg5():
        n = 2_000_000_000
        x = torch.empty(n, device=dev)
        CH = 1 << 27

        def fill(dst, r):
            for c, s0 in enumerate(range(0, n, CH)):
                g = torch.Generator(device=dev).manual_seed(r * 100003 + c)
                dst[s0:s0 + CH] = torch.randn(min(CH, n - s0), device=dev, generator=g)
        F8 = Operands.FLOAT_OPERAND(codec="fp8")
        fill(x, rank)
        comm.allreduceArray(x, F8, Operators.Float.SUM, 0, n)
        sync()
        num = den = 0.0
        for c, s0 in enumerate(range(0, 1 << 28, CH)):        # error on the first 1 GB (bounded cost)
            ref = torch.zeros(CH, dtype=torch.float64, device=dev)
            for j in range(p):
                g = torch.Generator(device=dev).manual_seed(j * 100003 + c)
                ref += torch.randn(CH, device=dev, generator=g).double()
            d = x[s0:s0 + CH].double() - ref
            num += float((d * d).sum())
            den += float((ref * ref).sum())
        rel = (num / max(den, 1e-300)) ** 0.5
        ms = _timed_p50(torch, lambda: comm.allreduceArray(x, F8, Operators.Float.SUM, 0, n, scale=1.0 / p), 3, sync)
        del x
        return {"ms": round(ms, 3), "rel_l2_error_vs_fp64": round(rel, 5), "exact": rel < 0.1,
                "busbw_gbps": round(8e9 / (ms * 1e-3) / 1e9 * 2 * (p - 1) / p, 2)}

    for name, fn in (("config3_rs_ag_4gb_bf16", cfg3), ("config4_sparse_200k_x64", cfg4),
                     ("config5_fp8_8gb", cfg5)):
        if not may_start(name):          # the extras' wall-time budget is spent (agreed)
            continue
        failed = 0.0
        try:
            out[name] = fn()
        except Exception as e:   # noqa: BLE001 — evidence only; the headline is already measured
            out[name] = {"error": str(e)[:200]}
            failed = 1.0
        torch.cuda.empty_cache()
        flag = torch.tensor([failed], dtype=torch.float64, device=agree_dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        if flag.item() > 0:
            break
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bytes", type=int, default=1_000_000_000)
    ap.add_argument("--algo", default=None, help="force device algorithm: rccl | a2a | ipc2z | ...")
    ap.add_argument("--codec", default=None, help="wire codec for the fp8-compressed config: fp8")
    ap.add_argument("--cpu", action="store_true", help="dry run of the launch/rendezvous path on CPU (gloo)")
    ap.add_argument("--no-autotune", action="store_true",
                    help="skip the warm-up schedule autotune (RCCL vs IPC two-shot vs a2a) for N>1")
    ap.add_argument("--autotune-iters", type=int, default=5, help="timed calls per autotune candidate")
    ap.add_argument("--alloc", choices=("register", "memalloc", "plain"), default="register")
    ap.add_argument("--no-register", action="store_true", help="= --alloc plain")
    ap.add_argument("--no-verify", action="store_true", help="skip the post-run exact-pattern check")
    ap.add_argument("--no-rccl-baseline", action="store_true", help="skip the equal-method RCCL baseline")
    ap.add_argument("--no-tier-sweep", action="store_true",
                    help="N>1: skip the untimed per-size schedule sweep (4 KiB .. 64 MiB) run after the timed steps")
    ap.add_argument("--sweep-sizes", default="4096,65536,262144,1048576,4194304,16777216,67108864",
                    help="N>1: comma-separated byte sizes of the allreduce schedule sweep, in order")
    ap.add_argument("--no-rooted-sweep", action="store_true", help="N>1: skip the rooted collectives' sweep")
    ap.add_argument("--no-configs", action="store_true",
                    help="N>1: skip the untimed BASELINE configs 3-5 (4 GB bf16 RS+AG, sparse map, 8 GB fp8) run last")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed call returned as DIR/<name>.npy (float32)")
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline does not need: p50 / p99 pass, self-verification, RCCL "
                         "baseline, topology probe, schedule sweeps, BASELINE configs 3-5")
    args = ap.parse_args()
    if args.no_register:
        args.alloc = "plain"
    if args.algo:
        os.environ["MP4X_DEVICE_ALGO"] = args.algo
    if args.dump_outputs:
        args.dump_outputs = os.path.abspath(args.dump_outputs)
    _leave_unwritable_cwd()

    import torch
    import torch.distributed as dist
    from mp4x import Operands, Operators
    from mp4x.launch import init_from_env

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("MP4X_DEVICE_INDEX", os.environ.get("LOCAL_RANK", "0")))
    if world != args.gpus:
        print(f"warning: --gpus {args.gpus} but WORLD_SIZE {world}", file=sys.stderr)
    if args.cpu:
        dev = torch.device("cpu")
        torch.cuda.synchronize = lambda *a, **k: None
        torch.cuda.Event = _CpuEvent
    else:
        torch.cuda.set_device(local)
        dev = torch.device("cuda", local)

    comm = init_from_env(heartbeat=False)
    p = comm.getSlaveNum()
    n = args.bytes // 4
    operand = Operands.FLOAT_OPERAND(codec=args.codec)
    op = Operators.Float.SUM
    scale = 1.0 / p

    registered = False
    if p > 1 and not args.cpu:
        comm.device  # bring up the RCCL communicator before anything is timed
    if p > 1 and not args.cpu and args.alloc == "memalloc":
        buf = comm.memAlloc(n, torch.float32)
        registered = comm.device._ipc_obj is not None and comm.device._ipc_obj.registered(buf) is not None
    else:
        buf = torch.empty(n, device=dev, dtype=torch.float32)
    g = torch.Generator(device=dev)
    g.manual_seed(1234 + rank)
    buf.normal_(generator=g)
    out = torch.empty_like(buf) if p == 1 else None

    def step():
        if p == 1:
            comm.allreduceArray(buf, operand, op, 0, n, out=out)
        else:
            comm.allreduceArray(buf, operand, op, 0, n, scale=scale)

    def sync_all():
        torch.cuda.synchronize()
        if p > 1:
            comm.peer_barrier() if args.cpu else comm.device.barrier()
            torch.cuda.synchronize()

    # host-side agreement tensors when gloo stands in for RCCL (the shared-GPU rehearsals): gloo
    # runs a CUDA tensor's collective on a fresh pool stream each call, every new stream takes
    # another hardware queue, and once the ranks' queues oversubscribe the GPU every barrier
    # kernel waits a scheduler time slice (~24-35 ms per call, profiles/r3/sweep/)
    agree_dev = "cpu" if args.cpu or (p > 1 and dist.get_backend() == "gloo") else dev

    def max_over_ranks(vals):
        t = torch.tensor(vals, dtype=torch.float64, device=agree_dev)
        if p > 1:
            if args.cpu:
                t = torch.from_numpy(comm.allreduceArray(t.numpy(), Operands.DOUBLE_OPERAND(),
                                                         Operators.Double.MAX, 0, len(vals)))
            else:
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return t.tolist()

    tuned = None
    if p > 1 and not args.cpu:
        if args.alloc == "register":
            registered = comm.registerBuffer(buf)   # collective; False on every rank alike
        if not (args.no_autotune or args.algo or args.codec):
            # untimed: measure every applicable schedule on a scratch tensor of this shape and
            # pin the fastest (all ranks agree: MAX over ranks); the timed steps run it in full
            tuned = {k: round(v * 1e3, 3) for k, v in
                     comm.device.autotune_allreduce(buf, op, iters=max(1, args.autotune_iters)).items()}
    for _ in range(args.warmup):
        step()

    wall = _time_steps(step, args.steps, sync_all)
    if args.dump_outputs:
        if rank == 0:
            _dump_output(torch, args.dump_outputs, "allreduce_out", out if p == 1 else buf)
        sync_all()              # no rank starts another in-place call while rank 0 still reads
    p50 = p99 = None
    if args.full:
        lat = _latency_pass(torch, step, args.steps, sync_all)     # ms, from the separate event pass
        wall, p50, p99 = max_over_ranks([wall, lat[len(lat) // 2], lat[min(len(lat) - 1, int(0.99 * len(lat)))]])
    else:
        wall = max_over_ranks([wall])[0]

    ms_per_step = wall * 1e3 / args.steps
    nbytes = n * 4
    algbw = nbytes / (ms_per_step * 1e-3) / 1e9
    factor = 2.0 * (p - 1) / p if p > 1 else 1.0
    busbw = algbw * factor
    algo = "k1_copy (out-of-place, 1 rank)" if p == 1 else ("host-tcp" if args.cpu else
                                  comm.device.select("allreduce", nbytes, Operators.Float.SUM, torch.float32, operand))
    if algo == "ipc2" and registered and not args.cpu and not comm.device._select_tuned:
        algo = "ipc2z"

    # ---- self-verification: the same call, same buffer, same pinned schedule, exact pattern
    verified, max_err = None, None
    if args.full and not args.no_verify:
        idt = torch.int32 if n < (1 << 31) else torch.int64
        i13 = torch.arange(n, device=dev, dtype=idt).remainder_(13)
        buf.copy_(i13 + rank)
        step()
        torch.cuda.synchronize()
        corrupt = os.environ.get("MP4X_BENCH_CORRUPT")      # test hook: a wrong element on one rank
        res = out if p == 1 else buf
        if corrupt is not None and int(corrupt) == rank:
            res[n // 2] += 1.0
        # exact answer in fp64: sum_j (i%13 + j) = p*(i%13) + p(p-1)/2, times the fused 1/p
        err = 0.0
        for lo in range(0, n, 1 << 26):                      # bounded fp64 temporaries
            hi = min(n, lo + (1 << 26))
            if p > 1:
                ex = (i13[lo:hi].double() * p + p * (p - 1) / 2) * scale
            else:                                            # the out-of-place copy
                ex = i13[lo:hi].double()
            err = max(err, float((res[lo:hi].double() - ex).abs().max()))
        del i13
        max_err = max_over_ranks([err])[0]
        # exact schedules: integers, then the 1/p scale (exact for p = 2/4/8); a lossy wire codec
        # (fp8: two e4m3 roundings, 2^-4 relative each) is held to its own bound
        tol = 1e-6 * 13 * p if not args.codec else 2.0 ** -3 * 13
        verified = bool(max_err <= tol)

    # ---- RCCL at equal method on the same buffer (N>1, GPU)
    rccl = None
    if args.full and p > 1 and not args.cpu and not args.no_rccl_baseline and not args.codec:
        eng = comm.device
        saved = eng.algo
        eng.algo = "rccl"
        try:
            for _ in range(max(1, args.warmup)):
                step()
            rwall, rlat = _measure(torch, step, args.steps, sync_all)
            rwall, rp50, rp99 = max_over_ranks([rwall, rlat[len(rlat) // 2],
                                                rlat[min(len(rlat) - 1, int(0.99 * len(rlat)))]])
            rms = rwall * 1e3 / args.steps
            rccl = {"rccl_ms_per_step": round(rms, 4), "rccl_p50_ms": round(rp50, 4), "rccl_p99_ms": round(rp99, 4),
                    "rccl_busbw_gbps": round(nbytes / (rms * 1e-3) / 1e9 * factor, 3)}
        finally:
            eng.algo = saved

    ref = REF_BUSBW_MBPS.get(p)
    topo = None
    if args.full and rank == 0 and not args.cpu:
        # which of the ranks' devices are one xGMI hop apart (native probe; one process per GPU
        # sees every device of the node, ranks 0..p-1 on devices 0..p-1)
        from mp4x.utils.topology import local_summary
        try:
            topo = local_summary(list(range(p)) if torch.cuda.device_count() >= p else [local])
            props = torch.cuda.get_device_properties(dev)
            topo = dict(topo or {}, gpu=props.name, gcn_arch=getattr(props, "gcnArchName", None),
                        cus=props.multi_processor_count, hbm_gib=round(props.total_memory / 2 ** 30, 1),
                        ranks_share_one_gpu=torch.cuda.device_count() < p)
        except Exception as e:   # noqa: BLE001 — evidence only
            topo = {"error": str(e)[:200]}
    selftest = None if (p == 1 or args.cpu) else comm.device.ipc_selftest
    ipc_inst = None if (p == 1 or args.cpu) else comm.device._ipc_obj
    ipc_info = None if ipc_inst is None else {"spin_s": ipc_inst.spin_s, "share": ipc_inst.share,
                                              "grid_caps": ipc_inst.grid_caps_summary()}

    def record(phase, tiers=None, configs=None, extras=None):
        stats = None if (p == 1 or args.cpu) else {k: v for k, v in comm.device.stats.items()
                                                   if k.startswith("allreduce")}
        probes = None if (p == 1 or args.cpu) else list(comm.device.probe_failures)
        return {
            "metric": METRIC,
            "value": round(busbw, 3),
            "unit": "GB/s",
            "n_gpus": p,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": round(busbw / (ref / 1e3), 2) if ref else None,
            "dtype": "fp32",
            "data": "synthetic (torch.randn per rank)",
            "config": {"model": f"allreduceArray float[{n}] ({nbytes / 1e9:g} GB), Operators.Float.SUM",
                       "global_batch": p, "seq_len": n, "parallelism": f"dp{p}",
                       "payload_bytes": nbytes, "algo": algo,
                       "alloc": args.alloc if p > 1 else "n/a", "registered": registered if p > 1 else "n/a",
                       "in_place": p > 1, "scale": scale if p > 1 else None, "autotune_ms": tuned,
                       "autotune_iters": args.autotune_iters, "ipc_selftest": selftest, "ipc": ipc_info,
                       "probe_failures": probes, "calls": stats, "tier_sweep_ms": tiers,
                       "baseline_configs": configs, "extras": extras, "topology": topo,
                       "tune_store": None if (p == 1 or args.cpu) else
                       {"path": comm.device.tune_path(), "loaded_at_start": comm.device.tune_loaded}},
            "verified": verified,
            "max_abs_err": max_err,
            "busbw_gbps_per_rank": round(busbw, 3),
            "aggregate_busbw_gbps": round(busbw * p, 3),
            "algbw_gbps": round(algbw, 3),
            "p50_ms": round(p50, 4) if p50 is not None else None,
            "p99_ms": round(p99, 4) if p99 is not None else None,
            "rccl_busbw_gbps": rccl["rccl_busbw_gbps"] if rccl else None,
            "rccl_p50_ms": rccl["rccl_p50_ms"] if rccl else None,
            "rccl_baseline": rccl,
            "busbw_factor": factor,
            "phase": phase,
            "note": ("p=1: nothing crosses a link (nccl-tests busbw factor 2(p-1)/p = 0), so this is "
                     "busbw := algbw of the out-of-place single-rank allreduce, a 1 GB HBM copy through K1; "
                     "N>=2 values are xGMI-link-bound and not comparable to N=1 as a scaling base"
                     if p == 1 else "value = busbw = algbw * 2(p-1)/p (nccl-tests convention, per rank); "
                                    "aggregate_busbw_gbps = p * busbw; rccl_* = the same call with RCCL forced"),
        }

    def finish():
        if args.alloc == "memalloc" and p > 1 and not args.cpu:
            comm.memFree(buf)
        comm.close(0)
        if p > 1 and dist.is_initialized():
            dist.destroy_process_group()

    # ---- a plain run ends here with its one result line
    if not args.full:
        if rank == 0:
            print(json.dumps(record("headline")), flush=True)
        finish()
        return

    # ---- the headline is measured, verified and next to RCCL: print it NOW, so nothing that runs
    # after it (sweeps, baseline configs) can lose it by hanging or overrunning the driver's timeout
    if rank == 0:
        print(json.dumps(record("headline")), flush=True)

    # ---- evidence after the headline, under ONE wall-time budget (MP4X_BENCH_EXTRA_S, default
    # 240 s): each stage starts only while the budget lasts (decided on the MAX elapsed over ranks,
    # so every rank starts or skips the same stages); what was skipped is recorded
    budget = float(os.environ.get("MP4X_BENCH_EXTRA_S", 240))
    t_extra = time.perf_counter()
    extras = {"budget_s": budget, "skipped": [], "seconds": None}
    if os.environ.get("MP4X_BENCH_TEST_HANG") == "extras" and rank == 0:
        # test hook: a stage that does not return in time (tests/test_launch_cpu.py); bounded, so a
        # run the test fails to kill still ends
        time.sleep(float(os.environ.get("MP4X_BENCH_TEST_HANG_S", 60)))

    def budget_left(stage) -> bool:
        if budget <= 0:
            extras["skipped"].append(stage)
            return False
        el = max_over_ranks([time.perf_counter() - t_extra])[0]
        if el >= budget:
            extras["skipped"].append(stage)
            return False
        return True

    def agreed_failure(failed) -> bool:
        # every rank stops together (a rank-local failure must not leave the others waiting in the
        # next stage's collectives)
        return max_over_ranks([failed])[0] > 0

    # measure every schedule at the size classes the IPC tiers are chosen for, so a multi-GPU run
    # records the tier boundaries on real links
    tiers = None
    gpu_extras = p > 1 and not args.cpu and not (args.algo or args.codec)
    if gpu_extras and not args.no_tier_sweep:
        tiers = {}
        for nb in [int(x) for x in args.sweep_sizes.split(",") if x.strip()]:
            if not budget_left(f"tier_sweep:{nb}"):
                continue
            failed = 0.0
            try:
                res = comm.device.autotune_allreduce(torch.empty(nb // 4, device=dev), op, iters=3)
                tiers[str(nb)] = {k: (round(v * 1e3, 4) if v != float("inf") else None) for k, v in res.items()}
            except Exception as e:   # noqa: BLE001 — evidence only; the headline is already printed
                tiers[str(nb)] = {"error": str(e)[:200]}
                failed = 1.0
            if agreed_failure(failed):
                break
        # the rooted collectives' schedules (RCCL vs IPC copy plans / two-shot) at sizes on both
        # sides of the IPC direct tier, recorded the same way
        rooted = {}
        for nb in () if args.no_rooted_sweep else (1 << 20, 16 << 20, 128 << 20):
            if not budget_left(f"rooted_sweep:{nb}"):
                continue
            failed = 0.0
            like = torch.empty(nb // 4, device=dev)
            row = {}
            try:
                for kind, fn in (("reduce", lambda: comm.device.autotune_reduce(like, op, root=p - 1)),
                                 ("broadcast", lambda: comm.device.autotune_broadcast(like, root=p - 1)),
                                 ("gather", lambda: comm.device.autotune_gather(like, root=p - 1)),
                                 ("scatter", lambda: comm.device.autotune_scatter(like, root=p - 1))):
                    row[kind] = {k: (round(v * 1e3, 4) if v != float("inf") else None) for k, v in fn().items()}
            except Exception as e:   # noqa: BLE001 — evidence only
                row["error"] = str(e)[:200]
                failed = 1.0
            rooted[str(nb)] = row
            if agreed_failure(failed):
                break
        tiers["rooted"] = rooted

    # the other BASELINE.json configs at this rank count (never timed with the headline): config 3
    # (RS + AG of a 4 GB bf16 memAlloc tensor), config 4 (sparse rows, 200k keys x float[64] per
    # rank, half shared), config 5 (8 GB f32 allreduce, fp8 wire codec)
    configs = None
    if gpu_extras and not args.no_configs:
        if budget_left("baseline_configs"):
            # a bounded IPC spin (60 s) for these evidence runs: a kernel that cannot complete raises
            # (recorded, every rank stops together) long before the watchdog's 600 s would end the job
            with comm.device.probing(float(os.environ.get("MP4X_BENCH_CONFIG_SPIN_S", 60))):
                configs = _baseline_configs(comm, torch, dist, p, rank, dev, agree_dev,
                                            lambda name: budget_left(name))
    extras["seconds"] = round(time.perf_counter() - t_extra, 3)
    if rank == 0:
        print(json.dumps(record("final", tiers, configs, extras)), flush=True)
    finish()
    if verified is False:
        print(f"bench: result NOT verified (max_abs_err {max_err})", file=sys.stderr, flush=True)
        sys.exit(RC_UNVERIFIED)


if __name__ == "__main__":
    main()
