#!/usr/bin/env python3
"""Measurement of pcr_thin (k_thin_runs, k_thin_mark, k_thin_flag, k_thin_totals, k_thin_write) on one GPU -- not the headline bench.

    python tools/bench_thin.py [--points 100000000] [--steps 20] [--warmup 3] [--layouts point_windows,words]
                               [--cells 128,330,930] [--out profiles/thin.json]

Per layout: the synthetic stream of the headline config, loaded, one frame drawn, then in ONE process on one box
  decode      `steps` pcr_decode_points calls of the whole stream between one pair of HIP events (tools/bench_decode.py's figure)
  depth       the HQS depth pass over the whole stream (pcr_kernel_timing_*, LOD 100 %, cull 0): a colourless decode + projection
  per cell and mode (first, center), `steps` calls between one event pair of each of
      count   both destinations NULL: phases one to three
      points  the kept records into a tensor of exactly their number
      rows    the records and their rows
    with points per voxel, runs / points, table_slots, and two ratios:
      ratio_to_model        time / (2 x depth pass + decode call): what the four phases would cost with free atomics
      speedup_over_torch    against what a user has today, measured beside it on the host clock: decode_points() of
                            everything, voxel keys, torch.unique(return_inverse), scatter_reduce(amin) of d2 << 40 | row, gather
The cells (lattice steps of the tile's millimetres) are chosen so that about 1, 8 and 64 points of the 1e8-point tile fall into a
voxel. Every result is compared with the torch alternative before it is timed. Prints one JSON line and writes it to --out.
A number that was not measured on the GPU is reported as "not measured".
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHUNK = 6553600                    # points per Morton-sorted chunk = 100 batches, as bench.py builds the headline stream
PPB = 65536
MODES = {"first": 0, "center": 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layouts", default="point_windows,words")
    ap.add_argument("--cells", default="128,330,930")
    ap.add_argument("--depth-frames", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thin.json"))
    args = ap.parse_args()

    import torch
    import pcrhpg24_amd as P
    from pcrhpg24_amd import _native as N
    if not torch.cuda.is_available():
        sys.exit("bench_thin.py measures on the GPU: none found")
    n = args.points
    cells = [int(c) for c in args.cells.split(",")]
    t0 = time.time()
    image, st = P.synth_encode(n, 0x5EED, 0, n, CHUNK, args.threads)
    f = P.HuffmanFile(image)
    nb = f.numBatches
    rec = {"what": "pcr_thin over the whole synthetic stream, no clip, origin (0, 0, 0)", "kernel_version": P.kernel_version(), "points_in": n,
           "points_decoded": nb * PPB, "batches": nb, "steps": args.steps, "warmup": args.warmup, "generate_s": round(time.time() - t0, 1),
           "cells": cells, "layouts": {}}
    print(f"stream of {nb} batches generated in {rec['generate_s']} s", file=sys.stderr, flush=True)
    dev = torch.device("cuda", 0)
    all_pts = torch.empty((nb * PPB, 4), dtype=torch.int32, device=dev)
    p = P.camera_orbit(-0.15, -0.57, 1500.0, (500.0, 500.0, 40.0), 1920, 1080)
    p.lod_percent, p.enable_frustum_culling = 100, 0

    def chk(ctx, rc, what):
        if rc:
            raise P.PcrError(f"{what} -> {rc}: {ctx.lib.pcr_last_error(ctx.h).decode()}")

    def torch_thin(ctx, cell, mode):
        """today's way: the whole cloud decoded, then one row per voxel by sorting 64-bit keys"""
        pts = ctx.decode_points(0, None, out=all_pts)
        d = pts[:, :3].to(torch.int64)
        v = torch.div(d, cell, rounding_mode="floor")
        row = torch.arange(pts.shape[0], dtype=torch.int64, device=dev)
        val = row
        if mode == "center":
            e = 2 * (d - v * cell) - (cell - 1)
            val = ((e * e).sum(dim=1) << 40) | row
        v = v - v.amin(dim=0)
        key = v[:, 0] | (v[:, 1] << 21) | (v[:, 2] << 42)
        uniq, inv = torch.unique(key, return_inverse=True)
        best = torch.full((uniq.shape[0],), (1 << 63) - 1, dtype=torch.int64, device=dev).scatter_reduce(0, inv, val, "amin")
        rows = torch.sort(best & ((1 << 40) - 1)).values
        out = pts[rows]
        torch.cuda.synchronize()
        return out, rows

    for name in args.layouts.split(","):
        ctx = P.Context(0)
        ctx.set_stream_layout({"point_windows": P.Context.LAYOUT_POINT_WINDOWS, "words": P.Context.LAYOUT_WORDS}[name])
        ctx.set_image_size(1920, 1080)
        ctx.stream_begin(f.header())
        for b0 in range(0, nb, 100):
            ctx.upload_batches(b0, [f.blob(b) for b in range(b0, min(b0 + 100, nb))])
        ctx.clear(); ctx.render_hqs_depth(p); ctx.synchronize()
        ctx.kernel_timing(1)
        for _ in range(args.depth_frames):
            ctx.clear(); ctx.render_hqs_depth(p)
        t_depth, _ = ctx.kernel_timing_read()
        ctx.kernel_timing(0)

        def timed(call):
            for _ in range(args.warmup):
                call()
            ctx.synchronize()
            ctx.timing_begin()
            for _ in range(args.steps):
                call()
            return ctx.timing_end() / args.steps

        t_decode = timed(lambda: chk(ctx, ctx.lib.pcr_decode_points(ctx.h, 0, -1, C.c_void_p(all_pts.data_ptr()), nb * PPB), "pcr_decode_points"))
        model = 2 * t_depth + t_decode
        row = {"decode_points_ms": round(t_decode, 4), "hqs_depth_pass_ms": round(t_depth, 4), "model_ms": round(model, 4), "cells": {}}
        ctx.batch_point_bounds()                            # (the exact boxes: once per context, tools/bench_select.py times it)
        for cell in cells:
            vox = P.as_voxels((0, 0, 0, cell))
            crow = {}
            for mode, m in MODES.items():
                if m == 1 and cell > N.THIN_MAX_CENTER_CELL:
                    continue
                cnt, tst = C.c_int64(), N.ThinStats()

                def call(points=None, rows=None, cap=0):
                    chk(ctx, ctx.lib.pcr_thin(ctx.h, 0, -1, C.byref(vox), None, m, C.c_void_p(points), C.c_void_p(rows), cap, C.byref(cnt), C.byref(tst)), "pcr_thin")

                call()
                k = cnt.value
                want, want_rows = torch_thin(ctx, cell, mode)
                out = torch.empty((k, 4), dtype=torch.int32, device=dev)
                out_rows = torch.empty(k, dtype=torch.int64, device=dev)
                torch.cuda.synchronize()
                call(out.data_ptr(), out_rows.data_ptr(), k)
                if want.shape[0] != k or not torch.equal(out, want) or not torch.equal(out_rows, want_rows):
                    sys.exit(f"{name} cell {cell} {mode}: pcr_thin differs from the torch alternative")
                del want, want_rows
                stats = tst.as_dict()
                r = {"kept": k, "points_per_voxel": round(stats["points_considered"] / max(k, 1), 3),
                     "runs_per_point": round(stats["runs"] / max(stats["points_considered"], 1), 4), "runs": stats["runs"], "table_slots": stats["table_slots"]}
                for label, a in (("count", (None, None, 0)), ("points", (out.data_ptr(), None, k)), ("rows", (out.data_ptr(), out_rows.data_ptr(), k))):
                    t = timed(lambda: call(*a))
                    r[label + "_ms"] = round(t, 4)
                    r[label + "_ratio_to_model"] = round(t / model, 3)
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    call(out.data_ptr(), None, k)
                host_ms = (time.perf_counter() - t0) * 1e3 / args.steps
                torch_thin(ctx, cell, mode)
                t0 = time.perf_counter()
                for _ in range(args.torch_reps):
                    torch_thin(ctx, cell, mode)
                t_alt = (time.perf_counter() - t0) * 1e3 / args.torch_reps
                r.update(points_host_ms=round(host_ms, 4), decode_plus_torch_unique_host_ms=round(t_alt, 4), speedup_over_torch=round(t_alt / host_ms, 2))
                crow[mode] = r
                print(f"{name} cell {cell} {mode}: {r}", file=sys.stderr, flush=True)
                del out, out_rows
                torch.cuda.empty_cache()
            row["cells"][str(cell)] = crow
        rec["layouts"][name] = row
        ctx.close()
    line = json.dumps(rec)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fo:
            json.dump(rec, fo, indent=1)
    print(line)


if __name__ == "__main__":
    main()
