#!/usr/bin/env python3
"""Measurement of pcr_voxel_mean (pcr_thin's FIRST plan, then k_voxel_prefix, k_voxel_index, k_voxel_sum, k_voxel_finish) on one GPU
-- not the headline bench.

    python tools/bench_voxel_mean.py [--points 100000000] [--steps 20] [--warmup 3] [--layouts point_windows,words]
                                     [--cells 128,330,930] [--out profiles/voxel_mean.json]

Per layout: the synthetic stream of the headline config, loaded, one frame drawn, then in ONE process on one box, per cell, `steps`
calls between one pair of HIP events of each of
    count        all three destinations NULL: pcr_thin's phases one to three and nothing else
    points       the mean records into a tensor of exactly their number
    all          the records, the rows and the counts
and beside them, in the same process,
    thin_count / thin_rows   pcr_thin FIRST with both destinations NULL, and with records and rows
    torch        what a user has today, on the host clock: decode_points() of everything, voxel keys, torch.unique(return_inverse),
                 index_add_ of int64 sums, the same integer rounding, the order by scatter_reduce(amin) of the row
with points per voxel, runs / points, and
    ratio_to_thin_rows    all / thin_rows
    sums_ms               points - thin_count: the index pass, the colour-decoding sum pass with its atomics, the finish pass
    speedup_over_torch    torch / the `all` call on the host clock
Every result is compared with the torch alternative's records, rows and counts before it is timed. Prints one JSON line and writes
it to --out. A number that was not measured on the GPU is reported as "not measured".
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layouts", default="point_windows,words")
    ap.add_argument("--cells", default="128,330,930")
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_mean.json"))
    args = ap.parse_args()

    import torch
    import pcrhpg24_amd as P
    from pcrhpg24_amd import _native as N
    if not torch.cuda.is_available():
        sys.exit("bench_voxel_mean.py measures on the GPU: none found")
    n = args.points
    cells = [int(c) for c in args.cells.split(",")]
    t0 = time.time()
    image, st = P.synth_encode(n, 0x5EED, 0, n, CHUNK, args.threads)
    f = P.HuffmanFile(image)
    nb = f.numBatches
    rec = {"what": "pcr_voxel_mean over the whole synthetic stream, no clip, origin (0, 0, 0)", "kernel_version": P.kernel_version(), "points_in": n,
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

    def torch_mean(ctx, cell):
        """today's way: the whole cloud decoded, then sums per voxel by sorting 64-bit keys and scattering"""
        pts = ctx.decode_points(0, None, out=all_pts)
        d = pts[:, :3].to(torch.int64)
        v = torch.div(d, cell, rounding_mode="floor")
        r = d - v * cell
        lo = v.amin(dim=0)
        v = v - lo
        key = v[:, 0] | (v[:, 1] << 21) | (v[:, 2] << 42)
        del d, v
        uniq, inv = torch.unique(key, return_inverse=True)
        del key
        k = uniq.shape[0]
        row = torch.arange(pts.shape[0], dtype=torch.int64, device=dev)
        cnt = torch.zeros(k, dtype=torch.int64, device=dev).index_add_(0, inv, torch.ones_like(row))
        s = torch.zeros((k, 3), dtype=torch.int64, device=dev).index_add_(0, inv, r)
        del r
        col = pts[:, 3].to(torch.int64)
        cb = torch.stack([(col >> (8 * j)) & 255 for j in range(4)], dim=1)
        c = torch.zeros((k, 4), dtype=torch.int64, device=dev).index_add_(0, inv, cb)
        del col, cb
        first = torch.full((k,), (1 << 63) - 1, dtype=torch.int64, device=dev).scatter_reduce(0, inv, row, "amin")
        del inv, row
        n2 = 2 * cnt[:, None]
        corner = (torch.stack([uniq & 0x1FFFFF, (uniq >> 21) & 0x1FFFFF, uniq >> 42], dim=1) + lo) * cell
        pos = corner + torch.div(2 * s + cnt[:, None], n2, rounding_mode="floor")
        mc = torch.div(2 * c + cnt[:, None], n2, rounding_mode="floor")
        colour = mc[:, 0] | (mc[:, 1] << 8) | (mc[:, 2] << 16) | (mc[:, 3] << 24)
        colour = torch.where(colour >= 1 << 31, colour - (1 << 32), colour)
        order = torch.argsort(first)
        out = torch.cat([pos, colour[:, None]], dim=1).to(torch.int32)[order]
        rows, counts = first[order], cnt[order]
        torch.cuda.synchronize()
        return out, rows, counts

    for name in args.layouts.split(","):
        ctx = P.Context(0)
        ctx.set_stream_layout({"point_windows": P.Context.LAYOUT_POINT_WINDOWS, "words": P.Context.LAYOUT_WORDS}[name])
        ctx.set_image_size(1920, 1080)
        ctx.stream_begin(f.header())
        for b0 in range(0, nb, 100):
            ctx.upload_batches(b0, [f.blob(b) for b in range(b0, min(b0 + 100, nb))])
        ctx.clear(); ctx.render_hqs_depth(p); ctx.synchronize()

        def timed(call):
            for _ in range(args.warmup):
                call()
            ctx.synchronize()
            ctx.timing_begin()
            for _ in range(args.steps):
                call()
            return ctx.timing_end() / args.steps

        row = {"cells": {}}
        ctx.batch_point_bounds()                            # (the exact boxes: once per context, tools/bench_select.py times it)
        for cell in cells:
            vox = P.as_voxels((0, 0, 0, cell))
            cnt, tst = C.c_int64(), N.ThinStats()

            def call(points=None, rows=None, counts=None, cap=0):
                chk(ctx, ctx.lib.pcr_voxel_mean(ctx.h, 0, -1, C.byref(vox), None, C.c_void_p(points), C.c_void_p(rows), C.c_void_p(counts), cap, C.byref(cnt),
                                                C.byref(tst)), "pcr_voxel_mean")

            def thin(points=None, rows=None, cap=0):
                chk(ctx, ctx.lib.pcr_thin(ctx.h, 0, -1, C.byref(vox), None, N.THIN_FIRST, C.c_void_p(points), C.c_void_p(rows), cap, C.byref(cnt), None), "pcr_thin")

            call()
            k = cnt.value
            want, want_rows, want_counts = torch_mean(ctx, cell)
            out = torch.empty((k, 4), dtype=torch.int32, device=dev)
            out_rows = torch.empty(k, dtype=torch.int64, device=dev)
            out_counts = torch.empty(k, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            call(out.data_ptr(), out_rows.data_ptr(), out_counts.data_ptr(), k)
            if want.shape[0] != k or not torch.equal(out, want) or not torch.equal(out_rows, want_rows) or not torch.equal(out_counts, want_counts):
                sys.exit(f"{name} cell {cell}: pcr_voxel_mean differs from the torch alternative")
            thin(out.data_ptr(), out_rows.data_ptr(), k)
            if not torch.equal(out_rows, want_rows):
                sys.exit(f"{name} cell {cell}: pcr_thin differs from the torch alternative")
            del want, want_rows, want_counts
            stats = tst.as_dict()
            r = {"voxels": k, "points_per_voxel": round(stats["points_considered"] / max(k, 1), 3),
                 "runs_per_point": round(stats["runs"] / max(stats["points_considered"], 1), 4), "runs": stats["runs"], "table_slots": stats["table_slots"]}
            r["count_ms"] = round(timed(lambda: call()), 4)
            r["points_ms"] = round(timed(lambda: call(out.data_ptr(), None, None, k)), 4)
            r["all_ms"] = round(timed(lambda: call(out.data_ptr(), out_rows.data_ptr(), out_counts.data_ptr(), k)), 4)
            r["thin_count_ms"] = round(timed(lambda: thin()), 4)
            r["thin_rows_ms"] = round(timed(lambda: thin(out.data_ptr(), out_rows.data_ptr(), k)), 4)
            r["ratio_to_thin_rows"] = round(r["all_ms"] / r["thin_rows_ms"], 3)
            r["sums_ms"] = round(r["points_ms"] - r["thin_count_ms"], 4)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                call(out.data_ptr(), out_rows.data_ptr(), out_counts.data_ptr(), k)
            host_ms = (time.perf_counter() - t0) * 1e3 / args.steps
            torch_mean(ctx, cell)
            t0 = time.perf_counter()
            for _ in range(args.torch_reps):
                torch_mean(ctx, cell)
            t_alt = (time.perf_counter() - t0) * 1e3 / args.torch_reps
            r.update(all_host_ms=round(host_ms, 4), decode_plus_torch_host_ms=round(t_alt, 4), speedup_over_torch=round(t_alt / host_ms, 2))
            row["cells"][str(cell)] = r
            print(f"{name} cell {cell}: {r}", file=sys.stderr, flush=True)
            del out, out_rows, out_counts
            torch.cuda.empty_cache()
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
