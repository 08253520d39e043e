#!/usr/bin/env python3
"""Measurement of pcr_ground_filter and pcr_select_height on one GPU -- not the headline bench.

    python tools/bench_ground.py [--points 100000000] [--steps 20] [--warmup 3] [--layouts point_windows,words]
                                 [--out profiles/ground.json]

Per layout: the synthetic stream of the headline config, loaded, one frame drawn, then in ONE process on one box
  filter   on a grid of 50 cm cells (2000 x 2000) and on one of 12.3 cm cells (8131 x 8131, just under PCR_GRID_MAX_CELLS): the
           lowest-point plane of the stream (grid_accumulate + grid_unpack, not timed), then `steps` pcr_ground_filter calls with 5
           steps (radii 1 .. 16) between one pair of HIP events -- the whole call, the call with fill_rounds = 0 (morphology, flags
           and classes) and their difference (the fill) -- beside the bound passes x 8 bytes x cells / copy rate with the copy rate
           measured in the same process (a morphology step is 4 passes and the flag pass, then the class pass; a fill round is one)
  heights  pcr_select_height over the 50 cm ground plane, count-only and records, for a ground-only range (|h| <= 30 cm) and a
           vegetation range (2 m .. 50 m), beside pcr_select_box of the grid's box and beside today's alternative:
           Context.decode_points() of everything plus a torch gather and mask (host clock around calls that end in a synchronise)
Every timed result is compared with that alternative's first. No ratio is fixed in advance. Prints one JSON line and writes it
to --out. A number that was not measured on the GPU is reported as "not measured".
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
GRIDS = {                          # origin x, y, cell, width, height in the tile's millimetres
    "cells_2000x2000": (0, 0, 500, 2000, 2000),
    "cells_8131x8131": (0, 0, 123, 8131, 8131),
}
RADII, THRESHOLDS = (1, 2, 4, 8, 16), (150, 450, 750, 1350, 2500)
RANGES = {"ground": (-300, 300), "vegetation": (2000, 50000)}
INT32_MIN = -(1 << 31)
PIECE = 1 << 24                    # rows per boolean-index call of the torch alternative


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layouts", default="point_windows,words")
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ground.json"))
    args = ap.parse_args()

    import torch
    import pcrhpg24_amd as P
    from pcrhpg24_amd import _native as N
    if not torch.cuda.is_available():
        sys.exit("bench_ground.py measures on the GPU: none found")
    n = args.points
    t0 = time.time()
    image, st = P.synth_encode(n, 0x5EED, 0, n, CHUNK, args.threads)
    f = P.HuffmanFile(image)
    nb = f.numBatches
    rec = {"what": "pcr_ground_filter and pcr_select_height over the whole synthetic stream", "kernel_version": P.kernel_version(), "points_in": n,
           "points_decoded": nb * PPB, "batches": nb, "steps": args.steps, "warmup": args.warmup, "generate_s": round(time.time() - t0, 1),
           "grids": {k: list(v) for k, v in GRIDS.items()}, "radii": list(RADII), "thresholds": list(THRESHOLDS), "ranges": {k: list(v) for k, v in RANGES.items()},
           "layouts": {}}
    dev = torch.device("cuda", 0)
    all_pts = torch.empty((nb * PPB, 4), dtype=torch.int32, device=dev)
    p = P.camera_orbit(-0.15, -0.57, 1500.0, (500.0, 500.0, 40.0), 1920, 1080)
    p.lod_percent, p.enable_frustum_culling = 100, 0

    def chk(ctx, rc, what):
        if rc:
            raise P.PcrError(f"{what} -> {rc}: {ctx.lib.pcr_last_error(ctx.h).decode()}")

    def torch_heights(ctx, grid, ground, lo, hi):
        """decode_points + gather + mask: the selected records, as a user does it today."""
        ox, oy, cell, w, h = grid
        pts = ctx.decode_points(0, None, out=all_pts)
        x, y = pts[:, 0].to(torch.int64), pts[:, 1].to(torch.int64)
        cx, cy = (x - ox) // cell, (y - oy) // cell
        m = (x >= ox) & (y >= oy) & (cx < w) & (cy < h)
        g = ground.view(-1).to(torch.int64)[(cx + cy * w).clamp_(0, w * h - 1)]
        d = pts[:, 2].to(torch.int64) - g
        sel = m & (g != INT32_MIN) & (d >= lo) & (d <= hi)
        # (in pieces of 2^24 rows: one boolean index over the 1e8 rows came back with 2^26 zeroed rows on the one full-size attempt)
        out = torch.cat([pts[a:a + PIECE][sel[a:a + PIECE]] for a in range(0, pts.shape[0], PIECE)])
        torch.cuda.synchronize()
        return out

    for name in args.layouts.split(","):
        ctx = P.Context(0)
        ctx.set_stream_layout({"point_windows": P.Context.LAYOUT_POINT_WINDOWS, "words": P.Context.LAYOUT_WORDS}[name])
        ctx.set_image_size(1920, 1080)
        ctx.stream_begin(f.header())
        for b0 in range(0, nb, 100):
            ctx.upload_batches(b0, [f.blob(b) for b in range(b0, min(b0 + 100, nb))])
        ctx.clear(); ctx.render_hqs_depth(p); ctx.synchronize()
        _, copy_gbps = ctx.measure_hbm()

        def timed(call):
            for _ in range(args.warmup):
                call()
            ctx.synchronize()
            ctx.timing_begin()
            for _ in range(args.steps):
                call()
            return ctx.timing_end() / args.steps

        ctx.batch_point_bounds()                                            # the exact boxes: cached from here on
        row = {"copy_gbps": round(copy_gbps, 1), "filter": {}, "heights": {}}
        ground_small = None
        for label, grid in GRIDS.items():
            g = P.as_grid(grid)
            cells = g.width * g.height
            words = torch.empty(cells, dtype=torch.int64, device=dev)
            ctx.grid_clear(grid, bottom=words)
            ctx.grid_accumulate(grid, bottom=words)
            lowest, _ = ctx.grid_unpack(grid, words, N.GRID_BOTTOM)
            del words
            ground = torch.empty_like(lowest)
            gst = N.GroundStats()
            r = {}
            for what, rounds in (("whole", N.GROUND_MAX_FILL), ("morphology", 0)):
                gp = P.GroundParams(RADII, THRESHOLDS, rounds)

                def call():
                    chk(ctx, ctx.lib.pcr_ground_filter(ctx.h, C.byref(g), C.byref(gp), C.c_void_p(lowest.data_ptr()), C.c_void_p(ground.data_ptr()), None,
                                                       C.byref(gst)), "pcr_ground_filter")
                r[f"{what}_ms"] = round(timed(call), 4)
                if what == "whole":
                    r.update(gst.as_dict())
                    if label == "cells_2000x2000":
                        ground_small = ground.clone()
                        torch.cuda.synchronize()                            # (the next call writes `ground` on the context's stream)
            passes_m, passes_f = 5 * len(RADII) + 1, r["fill_rounds"] + (1 if r["cells_unfilled"] else 0)
            bound = lambda passes: passes * 8.0 * cells / (copy_gbps * 1e9) * 1e3
            r["fill_ms"] = round(r["whole_ms"] - r["morphology_ms"], 4)
            r["morphology_bound_ms"], r["fill_bound_ms"] = round(bound(passes_m), 4), round(bound(passes_f), 4)
            r["morphology_over_bound"] = round(r["morphology_ms"] / bound(passes_m), 2)
            r["fill_over_bound"] = round(r["fill_ms"] / bound(passes_f), 2) if passes_f else "not measured"
            row["filter"][label] = r
            del lowest, ground

        grid = GRIDS["cells_2000x2000"]
        g = P.as_grid(grid)
        box = P.as_box(((grid[0], grid[1], INT32_MIN), (grid[0] + grid[2] * grid[3] - 1, grid[1] + grid[2] * grid[4] - 1, (1 << 31) - 1)))
        cnt, hst, sst = C.c_int64(), N.HeightStats(), N.SelectStats()
        t_box_count = timed(lambda: chk(ctx, ctx.lib.pcr_select_box(ctx.h, 0, -1, C.byref(box), None, 0, C.byref(cnt), C.byref(sst)), "pcr_select_box"))
        t_box = timed(lambda: chk(ctx, ctx.lib.pcr_select_box(ctx.h, 0, -1, C.byref(box), C.c_void_p(all_pts.data_ptr()), nb * PPB, C.byref(cnt), C.byref(sst)),
                                  "pcr_select_box"))
        row["select_box"] = {"count_only_ms": round(t_box_count, 4), "records_ms": round(t_box, 4), "records": cnt.value, **sst.as_dict()}
        for label, (lo, hi) in RANGES.items():
            want = torch_heights(ctx, grid, ground_small, lo, hi)
            got = ctx.select_height(grid, ground_small, lo, hi)
            if not torch.equal(got, want):
                if got.shape == want.shape:
                    rows = (got != want).any(dim=1).nonzero().view(-1)
                    print(f"{rows.numel()} rows differ, first {rows[:4].tolist()}: {got[rows[:4]].tolist()} against {want[rows[:4]].tolist()}", file=sys.stderr)
                sys.exit(f"{name} {label}: select_height differs from decode_points + gather + mask ({got.shape[0]} against {want.shape[0]} records)")
            nrec = want.shape[0]
            del want, got
            out = torch.empty((nrec, 4), dtype=torch.int32, device=dev)
            args_c = (ctx.h, 0, -1, C.byref(g), C.c_void_p(ground_small.data_ptr()), None, lo, hi, 0)
            t_count = timed(lambda: chk(ctx, ctx.lib.pcr_select_height(*args_c, None, None, 0, C.byref(cnt), C.byref(hst)), "pcr_select_height"))
            t_rec = timed(lambda: chk(ctx, ctx.lib.pcr_select_height(*args_c, C.c_void_p(out.data_ptr()) if nrec else None, None, nrec, C.byref(cnt), C.byref(hst)),
                                      "pcr_select_height"))
            t0 = time.perf_counter()
            for _ in range(args.torch_reps):
                torch_heights(ctx, grid, ground_small, lo, hi)
            t_alt = (time.perf_counter() - t0) * 1e3 / args.torch_reps
            row["heights"][label] = {"records": nrec, "count_only_ms": round(t_count, 4), "records_ms": round(t_rec, 4),
                                     "count_only_over_select_box": round(t_count / t_box_count, 3), "records_over_select_box": round(t_rec / t_box, 3),
                                     "decode_plus_torch_gather_host_ms": round(t_alt, 4), "speedup_over_decode_plus_gather": round(t_alt / t_rec, 1),
                                     **hst.as_dict()}
            del out
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
