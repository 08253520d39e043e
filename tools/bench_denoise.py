#!/usr/bin/env python3
"""Measurement of pcr_denoise (k_thin_runs, k_denoise_clear, k_denoise_count, k_denoise_verdict, k_denoise_flag, k_thin_totals,
k_thin_write) on one GPU -- not the headline bench.

    python tools/bench_denoise.py [--points 100000000] [--steps 20] [--warmup 3] [--layouts point_windows,words]
                                  [--cells 128,330,930] [--out profiles/denoise.json]

Per layout: the synthetic stream of the headline config, loaded, one frame drawn, then in ONE process on one box, per cell:
  max_count   the median of N27 over all points, computed once with torch (about half of the points are isolated)
  per mode (keep, isolated), `steps` calls between one event pair of each of
      count   both destinations NULL: everything but the write
      points  the records into a tensor of exactly their number
      rows    the records and their rows
  thin_first  pcr_thin PCR_THIN_FIRST at the same cell, the same three figures, measured beside it: the call this one was built on
              (one decode pass and one table scan fewer, one atomic per run as well); `ratio_to_thin` = points / thin's points
  speedup_over_torch  against what a user has today, on the host clock: decode_points() of everything, voxel keys, torch.unique
                      with counts, 27 searchsorted lookups, a gather
Every result is compared with the torch alternative before it is timed. Where the time goes is in `phases_ms`: the count call
under pcr_kernel_timing is not split per kernel, so the phases are differences -- count minus pcr_thin's count is the third decode
plus the verdict scan less k_thin_flag, points minus count is k_thin_write. Prints one JSON line and writes it to --out.
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
MODES = {"keep": 0, "isolated": 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layouts", default="point_windows,words")
    ap.add_argument("--cells", default="128,330,930")
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise.json"))
    args = ap.parse_args()

    import torch
    import pcrhpg24_amd as P
    from pcrhpg24_amd import _native as N
    if not torch.cuda.is_available():
        sys.exit("bench_denoise.py measures on the GPU: none found")
    n = args.points
    cells = [int(c) for c in args.cells.split(",")]
    t0 = time.time()
    image, st = P.synth_encode(n, 0x5EED, 0, n, CHUNK, args.threads)
    f = P.HuffmanFile(image)
    nb = f.numBatches
    rec = {"what": "pcr_denoise over the whole synthetic stream, no clip, origin (0, 0, 0), max_count = the median N27", "kernel_version": P.kernel_version(),
           "points_in": n, "points_decoded": nb * PPB, "batches": nb, "steps": args.steps, "warmup": args.warmup, "generate_s": round(time.time() - t0, 1),
           "cells": cells, "layouts": {}}
    print(f"stream of {nb} batches generated in {rec['generate_s']} s", file=sys.stderr, flush=True)
    dev = torch.device("cuda", 0)
    all_pts = torch.empty((nb * PPB, 4), dtype=torch.int32, device=dev)
    p = P.camera_orbit(-0.15, -0.57, 1500.0, (500.0, 500.0, 40.0), 1920, 1080)
    p.lod_percent, p.enable_frustum_culling = 100, 0

    def chk(ctx, rc, what):
        if rc:
            raise P.PcrError(f"{what} -> {rc}: {ctx.lib.pcr_last_error(ctx.h).decode()}")

    def torch_n27(ctx, cell):
        """today's way: the whole cloud decoded, the points per voxel by sorting 64-bit keys, 27 lookups per voxel"""
        pts = ctx.decode_points(0, None, out=all_pts)
        v = torch.div(pts[:, :3].to(torch.int64), cell, rounding_mode="floor")
        v = v - v.amin(dim=0) + 1
        key = v[:, 0] | (v[:, 1] << 21) | (v[:, 2] << 42)
        del v
        uniq, inv, own = torch.unique(key, return_inverse=True, return_counts=True)
        del key
        total = torch.zeros_like(own)
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    other = uniq + (dx + (dy << 21) + (dz << 42))
                    at = torch.searchsorted(uniq, other).clamp_(max=uniq.shape[0] - 1)
                    total += torch.where(uniq[at] == other, own[at], torch.zeros_like(own))
        return pts, total[inv]

    PIECE = 1 << 24                 # rows per gather and per comparison: one indexing call over 1e8 rows (1.6 GB out) came back wrong in places

    def torch_denoise(ctx, cell, max_count, mode):
        pts, n27 = torch_n27(ctx, cell)
        rows = torch.nonzero((n27 <= max_count) == (mode == "isolated")).reshape(-1)
        out = torch.empty((rows.shape[0], 4), dtype=torch.int32, device=dev)
        for i in range(0, rows.shape[0], PIECE):
            out[i:i + PIECE] = pts[rows[i:i + PIECE]]
        torch.cuda.synchronize()
        return out, rows

    def same(a, b):
        return a.shape == b.shape and all(torch.equal(a[i:i + PIECE], b[i:i + PIECE]) for i in range(0, a.shape[0], PIECE))

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

        t_decode = timed(lambda: chk(ctx, ctx.lib.pcr_decode_points(ctx.h, 0, -1, C.c_void_p(all_pts.data_ptr()), nb * PPB), "pcr_decode_points"))
        row = {"decode_points_ms": round(t_decode, 4), "cells": {}}
        ctx.batch_point_bounds()                            # (the exact boxes: once per context, tools/bench_select.py times it)
        for cell in cells:
            vox = P.as_voxels((0, 0, 0, cell))
            _, n27 = torch_n27(ctx, cell)
            max_count = int(torch.sort(n27).values[n27.shape[0] // 2])
            del n27
            cnt, tst, dst = C.c_int64(), N.ThinStats(), N.DenoiseStats()

            def thin(points=None, rows=None, cap=0):
                chk(ctx, ctx.lib.pcr_thin(ctx.h, 0, -1, C.byref(vox), None, N.THIN_FIRST, C.c_void_p(points), C.c_void_p(rows), cap, C.byref(cnt), C.byref(tst)),
                    "pcr_thin")

            # the yardstick first: pcr_thin FIRST at the same cell
            thin()
            k = cnt.value
            out = torch.empty((k, 4), dtype=torch.int32, device=dev)
            out_rows = torch.empty(k, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            tr = {"kept": k}
            for label, a in (("count", (None, None, 0)), ("points", (out.data_ptr(), None, k)), ("rows", (out.data_ptr(), out_rows.data_ptr(), k))):
                tr[label + "_ms"] = round(timed(lambda: thin(*a)), 4)
            del out, out_rows
            crow = {"max_count": max_count, "thin_first": tr}
            for mode, m in MODES.items():
                def call(points=None, rows=None, cap=0):
                    chk(ctx, ctx.lib.pcr_denoise(ctx.h, 0, -1, C.byref(vox), None, max_count, m, C.c_void_p(points), C.c_void_p(rows), cap, C.byref(cnt),
                                                 C.byref(dst)), "pcr_denoise")

                call()
                k = cnt.value
                want, want_rows = torch_denoise(ctx, cell, max_count, mode)
                out = torch.empty((k, 4), dtype=torch.int32, device=dev)
                out_rows = torch.empty(k, dtype=torch.int64, device=dev)
                torch.cuda.synchronize()
                for a in ((None, None, 0), (out.data_ptr(), None, k), (out.data_ptr(), out_rows.data_ptr(), k)):    # every timed form is checked first
                    call(*a)
                    if cnt.value != want.shape[0] or (a[0] and not same(out, want)) or (a[1] and not same(out_rows, want_rows)):
                        sys.exit(f"{name} cell {cell} {mode}: pcr_denoise differs from the torch alternative")
                del want, want_rows
                stats = dst.as_dict()
                r = {"written": k, "points_isolated": stats["points_isolated"], "voxels": stats["voxels"], "voxels_isolated": stats["voxels_isolated"],
                     "points_per_voxel": round(stats["points_considered"] / max(stats["voxels"], 1), 3),
                     "runs_per_point": round(stats["runs"] / max(stats["points_considered"], 1), 4), "runs": stats["runs"], "table_slots": stats["table_slots"]}
                for label, a in (("count", (None, None, 0)), ("points", (out.data_ptr(), None, k)), ("rows", (out.data_ptr(), out_rows.data_ptr(), k))):
                    t = timed(lambda: call(*a))
                    r[label + "_ms"] = round(t, 4)
                    r[label + "_ratio_to_thin"] = round(t / tr[label + "_ms"], 3)
                r["phases_ms"] = {"count_over_thin_count": round(r["count_ms"] - tr["count_ms"], 4), "write": round(r["points_ms"] - r["count_ms"], 4),
                                  "thin_write": round(tr["points_ms"] - tr["count_ms"], 4)}
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    call(out.data_ptr(), None, k)
                host_ms = (time.perf_counter() - t0) * 1e3 / args.steps
                torch_denoise(ctx, cell, max_count, mode)
                t0 = time.perf_counter()
                for _ in range(args.torch_reps):
                    torch_denoise(ctx, cell, max_count, mode)
                t_alt = (time.perf_counter() - t0) * 1e3 / args.torch_reps
                r.update(points_host_ms=round(host_ms, 4), decode_plus_torch_host_ms=round(t_alt, 4), speedup_over_torch=round(t_alt / host_ms, 2))
                crow[mode] = r
                print(f"{name} cell {cell} max_count {max_count} {mode}: {r}", file=sys.stderr, flush=True)
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
