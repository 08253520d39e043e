#!/usr/bin/env python3
"""Measurement of the 10-10-10 methods ("loop_las_cuda", SURVEY 8f next row, and "loop_las_hqs") on one GPU — not the headline
bench.

    python tools/bench_las.py [--method loop_las_cuda|loop_las_hqs] [--points 100000000] [--order tiles|strips]
                              [--camera overview|closeup] [--steps 20]

Prints one JSON line: Mpoints/s of a frame (loop_las_cuda: clear + render + resolve; loop_las_hqs: clear + depth pass + colour
pass + resolve), the render kernel's HIP-event time and its HBM roofline fraction (algorithmic bytes = 4/8/12 B per point by
batch level + 64 B per drawn batch), and a full-size parity check against the oracle (loop_las_hqs: against the CPU reference
tests/las_hqs_ref.c, depth, sums and image; the checker, not the thing measured). loop_las_hqs also reports the depth pass's and
the colour pass's kernel times and the frame time.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--method", choices=["loop_las_cuda", "loop_las_hqs"], default="loop_las_cuda")
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--order", choices=["tiles", "strips"], default="tiles")
    ap.add_argument("--camera", choices=["overview", "closeup"], default="overview")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--cull", type=int, default=0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-parity", action="store_true")
    args = ap.parse_args()

    import pcrhpg24_amd as P
    seed, n = 0x5EED, args.points
    t0 = time.time()
    x, y, z, c = P.synth_points(n, seed, 0, n)
    las = P.synth_las_info(n, seed)
    if args.order == "tiles":            # spatially coherent file order: ~65 536-point square tiles
        side = max(1, int(round(1_000_000 / max(1.0, (n / 65536) ** 0.5))))
        key = (y // side).astype(np.int64) * 4096 + x // side
        idx = np.argsort(key, kind="stable")
        x, y, z, c = x[idx], y[idx], z[idx], c[idx]
    t_gen = time.time() - t0

    ctx = P.Context(0)
    ctx.set_image_size(args.width, args.height)
    t0 = time.time()
    q = P.las_quantize(x, y, z, c, las)
    t_quant = time.time() - t0
    t0 = time.time()
    ctx.las_begin(n)
    step_b = 100
    nb = len(q[0])
    XB = type(q[0][0])
    for b0 in range(0, nb, step_b):
        b1 = min(nb, b0 + step_b)
        sub = (XB * (b1 - b0)).from_buffer(q[0], b0 * 64)
        ctx.las_upload(b0, sub, *(a[b0 * 65536:b1 * 65536] for a in q[1:]))
    t_load = time.time() - t0

    if args.camera == "overview":
        p = P.camera_orbit(-0.15, -0.57, 1500.0, (500.0, 500.0, 40.0), args.width, args.height)
    else:
        p = P.camera_orbit(-1.68, -0.39, 70.0, (300.0, 20.0, 45.0), args.width, args.height)
    p.enable_frustum_culling = args.cull

    hqs = args.method == "loop_las_hqs"

    def step():
        if hqs:
            ctx.clear(); ctx.render_las_hqs_depth(p); ctx.render_las_hqs_color(p); ctx.resolve_hqs(p)
        else:
            ctx.clear(); ctx.render_las(p); ctx.resolve_las(p)

    for _ in range(args.warmup):
        step()
    ctx.synchronize()
    # event pair around k_las_render of each timed step (pcr_kernel_timing_*); loop_las_hqs: every second launch, the depth pass's
    ctx.kernel_timing(2 if hqs else 1)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    ctx.synchronize()
    elapsed = time.perf_counter() - t0
    st = ctx.stats()
    kernel_ms, _ = ctx.kernel_timing_read()
    ctx.kernel_timing(False)
    passes = None
    if hqs:
        # the colour pass alone, repeated over one depth pass (its sums pile up; the work per launch is the same)
        ctx.clear(); ctx.render_las_hqs_depth(p)
        ctx.kernel_timing(1)
        for _ in range(args.steps):
            ctx.render_las_hqs_color(p)
        color_ms, _ = ctx.kernel_timing_read()
        ctx.kernel_timing(False)
        alg_color = ctx.las_algorithmic_bytes
        ctx.clear(); ctx.render_las_hqs_depth(p)
        alg = ctx.las_algorithmic_bytes
        passes = {"depth_kernel_ms": round(kernel_ms, 4), "color_kernel_ms": round(color_ms, 4),
                  "frame_ms": round(1e3 * elapsed / args.steps, 4), "color_algorithmic_bytes": alg_color,
                  "frame": "clear + k_las_prepass + k_las_render<true> + k_las_prepass + k_las_render_color + k_resolve<true>"}
    else:
        alg = ctx.las_algorithmic_bytes
    achieved = alg / (kernel_ms * 1e-3) / 1e9
    parity = None
    if not args.no_parity:
        from tests import oracle
        if hqs:
            from tests import las_hqs_ref
            ctx.clear(); ctx.render_las_hqs_depth(p); ctx.render_las_hqs_color(p); ctx.resolve_hqs(p)
            t0 = time.perf_counter()
            ofb, ost = las_hqs_ref.render_depth(*q[:4], p)
            org, oba, _ = las_hqs_ref.render_color(*q, p, ofb)
            cpu_s = time.perf_counter() - t0
            rg, ba = ctx.read_accum(full=True)
            parity = bool(np.array_equal(ctx.read_framebuffer(full=True), ofb) and np.array_equal(rg, org) and np.array_equal(ba, oba)
                          and np.array_equal(ctx.read_rgba(), oracle.resolve_hqs(p, ofb, org, oba))) and ost == ctx.stats()
        else:
            ctx.clear(); ctx.render_las(p)
            t0 = time.perf_counter()
            ofb, ost = oracle.render_las(*q[:4], p)
            cpu_s = time.perf_counter() - t0
            parity = bool(np.array_equal(ctx.read_framebuffer(full=True), ofb)) and ost == ctx.stats()
    out = {"metric": "Mpoints/s rasterized @%dx%d (%s, 10-10-10)" % (args.width, args.height, args.method),
           "value": round(st["points_iterated"] / (elapsed / args.steps) / 1e6, 3), "unit": "Mpoints/s",
           "ms_per_step": round(1e3 * elapsed / args.steps, 4), "steps": args.steps, "warmup": args.warmup,
           "config": {"workload": "%d synthetic points in %s order, %dx%d, camera %s, cull=%d" %
                                  (n, args.order, args.width, args.height, args.camera, args.cull),
                      "batches": nb, "points_per_step": st["points_iterated"], "generate_s": round(t_gen, 2),
                      "quantize_s": round(t_quant, 2), "load_s": round(t_load, 2)},
           "roofline": {"bound": "hbm", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": round(achieved / HBM_PEAK_GBS, 5), "traffic": None, "kernel": "k_las_render<true>" if hqs else "k_las_render",
                        "kernel_ms": round(kernel_ms, 4), "algorithmic_bytes": alg,
                        "bytes_per_point": round(alg / max(1, st["points_iterated"]), 3)},
           "parity_full_size": parity}
    if passes is not None:
        out["passes"] = passes
    if parity is not None:
        out["cpu_baseline"] = {"value": round(ost["points_iterated"] / cpu_s / 1e6, 3), "unit": "Mpoints/s", "cores": 1,
                               "kind": "port", "sample": "whole workload, %s, %.1f s" % ("tests/las_hqs_ref.c depth + colour" if hqs else "oracle/pcr_oracle.c pcr_oracle_render_las", cpu_s)}
    print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
