#!/usr/bin/env python3
"""Measurement of pcr_grid_accumulate (k_grid) on one GPU -- not the headline bench.

    python tools/bench_grid.py [--points 100000000] [--steps 20] [--warmup 3] [--layouts point_windows,words]
                               [--out profiles/grid.json]

Per layout: the synthetic stream of the headline config, loaded, one frame drawn, then in ONE process on one box
  decode       `steps` pcr_decode_points calls of the whole stream between one pair of HIP events (tools/bench_decode.py's figure)
  coarse       a grid of 16 m cells over the tile (63 x 63 cells: whatever a batch's box, its footprint is at most 3969 cells, so
               every batch is windowed): `steps` pcr_grid_accumulate calls between one event pair, top only and all three planes
  coarse_direct  the same grid with PCR_GRID_NO_WINDOW: every batch goes straight to global atomics
  fine         a grid of 12.5 cm cells (8000 x 8000): every batch covers more than PCR_GRID_WINDOW_CELLS cells and is direct anyway
and beside each, today's alternative: Context.decode_points() of everything + torch scatter_reduce / bincount to the same planes
(host clock around calls that end in a synchronise). Every grid is compared with that alternative before it is timed.
The expectation checked: the all-windowed call reads and decodes what pcr_decode_points does and stores almost nothing, so it takes
at most --slack (1.10) x the pcr_decode_points call of the same process. Prints one JSON line and writes it to --out.
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
GRIDS = {                          # origin x, y, cell, width, height in the tile's millimetres
    "coarse": (0, 0, 16_000, 63, 63),
    "fine": (0, 0, 125, 8000, 8000),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layouts", default="point_windows,words")
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--slack", type=float, default=1.10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid.json"))
    args = ap.parse_args()

    import torch
    import pcrhpg24_amd as P
    from pcrhpg24_amd import _native as N
    if not torch.cuda.is_available():
        sys.exit("bench_grid.py measures on the GPU: none found")
    n = args.points
    t0 = time.time()
    image, st = P.synth_encode(n, 0x5EED, 0, n, CHUNK, args.threads)
    f = P.HuffmanFile(image)
    nb = f.numBatches
    rec = {"what": "pcr_grid_accumulate over the whole synthetic stream", "kernel_version": P.kernel_version(), "points_in": n,
           "points_decoded": nb * PPB, "batches": nb, "steps": args.steps, "warmup": args.warmup, "generate_s": round(time.time() - t0, 1),
           "slack": args.slack, "grids": {k: list(v) for k, v in GRIDS.items()}, "layouts": {}}
    dev = torch.device("cuda", 0)
    all_pts = torch.empty((nb * PPB, 4), dtype=torch.int32, device=dev)
    p = P.camera_orbit(-0.15, -0.57, 1500.0, (500.0, 500.0, 40.0), 1920, 1080)
    p.lod_percent, p.enable_frustum_culling = 100, 0
    sign = torch.tensor(-(1 << 63), dtype=torch.int64, device=dev)

    def chk(ctx, rc, what):
        if rc:
            raise P.PcrError(f"{what} -> {rc}: {ctx.lib.pcr_last_error(ctx.h).decode()}")

    def torch_planes(ctx, grid, all_three):
        """decode_points + scatter_reduce to the same planes (top as the bits of the unsigned max; bottom, count with all_three)."""
        ox, oy, cell, w, h = grid
        pts = ctx.decode_points(0, None, out=all_pts)
        x, y = pts[:, 0].to(torch.int64), pts[:, 1].to(torch.int64)
        cx, cy = (x - ox) // cell, (y - oy) // cell
        m = (x >= ox) & (y >= oy) & (cx < w) & (cy < h)
        idx = (cx + cy * w)[m]
        key = ((pts[:, 2].to(torch.int64) << 32) | (pts[:, 3].to(torch.int64) & 0xFFFFFFFF))[m]
        top = torch.full((w * h,), -(1 << 63), dtype=torch.int64, device=dev).scatter_reduce(0, idx, key, "amax") ^ sign
        bottom = count = None
        if all_three:
            bottom = torch.full((w * h,), (1 << 63) - 1, dtype=torch.int64, device=dev).scatter_reduce(0, idx, key, "amin") ^ sign
            count = torch.bincount(idx, minlength=w * h).to(torch.int32)
        torch.cuda.synchronize()
        return top, bottom, count

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
        ctx.batch_point_bounds()                                            # the exact boxes: cached from here on
        row = {"decode_points_ms": round(t_decode, 4)}
        for label, grid, flags in (("coarse", GRIDS["coarse"], 0), ("coarse_direct", GRIDS["coarse"], N.GRID_NO_WINDOW), ("fine", GRIDS["fine"], 0)):
            g = P.as_grid(grid)
            cells = g.width * g.height
            top = torch.empty(cells, dtype=torch.int64, device=dev)
            bottom, count = torch.empty_like(top), torch.empty(cells, dtype=torch.int32, device=dev)
            gst = N.GridStats()
            r = {}
            for planes, ptrs in (("top", (top, None, None)), ("all", (top, bottom, count))):
                args_c = [C.c_void_p(t.data_ptr()) if t is not None else None for t in ptrs]
                torch.cuda.synchronize()

                def call():
                    chk(ctx, ctx.lib.pcr_grid_accumulate(ctx.h, 0, -1, C.byref(g), None, *args_c, flags, C.byref(gst)), "pcr_grid_accumulate")

                chk(ctx, ctx.lib.pcr_grid_clear(ctx.h, C.byref(g), *args_c), "pcr_grid_clear")
                call()
                ctx.synchronize()
                want = torch_planes(ctx, grid, planes == "all")
                for got, w, what in zip(ptrs, want, ("top", "bottom", "count")):
                    if got is not None and not torch.equal(got, w):
                        sys.exit(f"{name} {label} {planes}: the {what} plane differs from decode_points + scatter_reduce")
                del want
                t_grid = timed(call)
                t0 = time.perf_counter()
                for _ in range(args.torch_reps):
                    torch_planes(ctx, grid, planes == "all")
                t_alt = (time.perf_counter() - t0) * 1e3 / args.torch_reps
                r[planes] = {"grid_ms": round(t_grid, 4), "ratio_to_decode_points": round(t_grid / t_decode, 3),
                             "decode_plus_torch_scatter_host_ms": round(t_alt, 4), "speedup_over_decode_plus_scatter": round(t_alt / t_grid, 1)}
            r.update(gst.as_dict())
            row[label] = r
            del top, bottom, count
        if row["coarse"]["batches_windowed"] != nb or row["coarse_direct"]["batches_direct"] != nb or row["fine"]["batches_direct"] != nb:
            sys.exit(f"{name}: the grids do not put the batches into the classes this measurement is about: {row}")
        for planes in ("top", "all"):
            row[f"windowed_over_direct_{planes}"] = round(row["coarse"][planes]["grid_ms"] / row["coarse_direct"][planes]["grid_ms"], 3)
            row[f"windowed_within_{args.slack}x_of_decode_{planes}"] = bool(row["coarse"][planes]["grid_ms"] <= args.slack * t_decode)
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
