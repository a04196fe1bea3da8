#!/usr/bin/env python3
"""The combine's backward (local half, no exchange) three ways on one GPU, one process:

fused   K11 (csrc/kernels/moe.hip k_moe_combine_bwd) through ``device_ops.moe_combine_backward``: one
        pass over the output gradient gives the scaled rows and the gate weights' gradient
parent  what ``_Combine.backward`` does with ``backward="torch"``: the K9 route scatter with
        ``row_scale``, then the gather / float32 product / sum / where of the weights' gradient in torch
copy    plain device copies of the bytes K11 has to move: the slot rows into a buffer of the gradient
        rows' size (read K*T*H, write K*T*H) and the gradient (read T*H; its write is counted too)

Per shape (T tokens x width, top K, dtype; ids uniform over ``--experts``): a call is timed as a batch
of ``--iters`` launches between two device events, the forms alternate in ``--rounds`` rounds and a row
gives the median of the rounds with their extremes.  ``bytes`` is what the form has to move (fused:
g once, rows once, g_rows once; copy: what it copies, read and written), ``peak_bytes`` is
``torch.cuda.max_memory_allocated`` of one call above what was allocated before it (outputs and
temporaries).  Prints one JSON line per row."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _batch_us(torch, call, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        call()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / iters


def _peak(torch, call):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = call()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=4096)
    ap.add_argument("--widths", default="7168,1024")
    ap.add_argument("--top-k", default="2,8")
    ap.add_argument("--dtypes", default="bfloat16,float32")
    ap.add_argument("--experts", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    import torch
    from mp4x.ops import device_ops as ops
    if not torch.cuda.is_available():
        raise SystemExit("bench/moe_combine_bwd.py needs a GPU")
    torch.cuda.set_device(0)
    T, E = a.tokens, a.experts
    for dtype in a.dtypes.split(","):
        dt = getattr(torch, dtype)
        for H in (int(x) for x in a.widths.split(",")):
            for K in (int(x) for x in a.top_k.split(",")):
                gen = torch.Generator(device="cuda").manual_seed(H + K)
                g = torch.randn(T, H, device="cuda", generator=gen).to(dt)
                w = torch.rand(T, K, device="cuda", generator=gen)
                ids = torch.randint(0, E, (T, K), device="cuda", generator=gen)
                rc = ops.moe_route_count(ids.view(-1), E)
                n = T * K
                back = torch.randn(n, H, device="cuda", generator=gen).to(dt)
                slots = ops.moe_route_scatter(rc, g, K, torch.empty_like(back), placed=n)
                dst_rows, dst_g = torch.empty_like(back), torch.empty_like(g)

                def fused():
                    return ops.moe_combine_backward(g, back, slots, w, T, K, max_slot=n - 1)

                def parent():
                    g_rows = torch.empty((n, H), dtype=dt, device="cuda")
                    ops.moe_route_scatter(rc, g, K, g_rows, row_scale=w, placed=n)
                    sl = slots.view(T, K)
                    y = back.reshape(back.shape[0], -1)[sl.clamp(min=0)].to(torch.float32)      # [T, K, H]
                    g_w = (g.reshape(T, 1, -1).to(torch.float32) * y).sum(-1)
                    g_w = torch.where(sl >= 0, g_w, torch.zeros_like(g_w)).view_as(w)
                    return g_rows, g_w

                def copy():
                    dst_rows.copy_(back)
                    dst_g.copy_(g)

                es = g.element_size()
                moved = (2 * n * H + T * H) * es
                forms = (("fused", fused, moved + 16 * n), ("parent", parent, None), ("copy", copy, (2 * n * H + 2 * T * H) * es))
                f_rows, f_w = fused()
                p_rows, p_w = parent()
                rows_equal = bool(torch.equal(f_rows.view(torch.uint8), p_rows.view(torch.uint8)))
                w_diff = float((f_w - p_w).abs().max() / p_w.abs().max())
                del f_rows, f_w, p_rows, p_w
                peak = {"fused": _peak(torch, fused), "parent": _peak(torch, parent), "copy": 0}
                for _, call, _ in forms:
                    for _ in range(3):
                        call()
                torch.cuda.synchronize()
                us = {f[0]: [] for f in forms}
                for _ in range(a.rounds):                    # the forms alternate: a drifting clock hits all of them
                    for form, call, _ in forms:
                        us[form].append(_batch_us(torch, call, a.iters))
                for form, _, nbytes in forms:
                    v = sorted(us[form])
                    med = v[len(v) // 2]
                    print(json.dumps({"gpus": 1, "tokens": T, "width": H, "top_k": K, "dtype": dtype, "experts": E,
                                      "form": form, "us_median_of_rounds": round(med, 2), "min_of_rounds": round(v[0], 2),
                                      "max_of_rounds": round(v[-1], 2), "bytes": nbytes,
                                      "eff_gbps": round(nbytes / med / 1e3, 1) if nbytes else None,
                                      "peak_bytes": peak[form], "g_rows_equal_parent": rows_equal,
                                      "g_weights_max_diff_over_max_abs": w_diff,
                                      "timed": f"{a.iters} calls between two device events, host launch cost and the "
                                               f"outputs' allocation included"}), flush=True)
                del back, dst_rows, dst_g


if __name__ == "__main__":
    main()
