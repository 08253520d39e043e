#!/usr/bin/env python3
"""Measurement of pcr_grid_quantiles (k_quant_*) on one GPU -- not the headline bench.

    python tools/bench_grid_quantiles.py [--points 100000000] [--steps 20] [--warmup 3] [--layouts point_windows,words]
                                         [--out profiles/grid_quantiles.json]

Per layout: the synthetic stream of the headline config, loaded, one frame drawn, then in ONE process on one box
  decode        `steps` pcr_decode_points calls of the whole stream between one pair of HIP events
  coarse        a grid of 16 m cells over the tile (63 x 63 cells: every batch is windowed, some 25 000 candidates a cell)
  coarse_direct the same grid with PCR_GRID_NO_WINDOW: one global atomic per candidate in the count and in the fill
  fine          a grid of 12.5 cm cells (8000 x 8000): every batch is direct anyway, a candidate or two a cell
each with num_q = 1 (p95), num_q = 8 and count-only, `steps` calls between one event pair (the call synchronises inside: the
figure includes that), and beside each pcr_grid_accumulate with all three planes, and today's alternative: Context.decode_points()
of everything + a torch sort by (cell, z) + a gather at the ranks (host clock around calls that end in a synchronise). Every timed
result is first compared with that alternative's planes.
Nothing is asserted about the times. The expectation stated: count and fill are two colourless decode passes plus 4 bytes stored
per candidate, so num_q = 1 should be within a small multiple of count-only; whether the windowed reservation beats the direct one,
and what the selection costs at a candidate or two and at 25 000 per cell, is what the run shows (`select_share` = 1 - the
quantile call without its selection, estimated as (num_q = 1) - (count-only) against num_q = 8).
Prints one JSON line and writes it to --out. A number that was not measured on the GPU is reported as "not measured".
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
Q1, Q8 = (9500,), (100, 500, 2500, 5000, 7500, 9500, 9900, 10000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layouts", default="point_windows,words")
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_quantiles.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import pcrhpg24_amd as P
    from pcrhpg24_amd import _native as N
    if not torch.cuda.is_available():
        sys.exit("bench_grid_quantiles.py measures on the GPU: none found")
    n = args.points
    t0 = time.time()
    image, st = P.synth_encode(n, 0x5EED, 0, n, CHUNK, args.threads)
    f = P.HuffmanFile(image)
    nb = f.numBatches
    rec = {"what": "pcr_grid_quantiles over the whole synthetic stream", "kernel_version": P.kernel_version(), "points_in": n,
           "points_decoded": nb * PPB, "batches": nb, "steps": args.steps, "warmup": args.warmup, "generate_s": round(time.time() - t0, 1),
           "q1": list(Q1), "q8": list(Q8), "grids": {k: list(v) for k, v in GRIDS.items()}, "layouts": {}}
    dev = torch.device("cuda", 0)
    all_pts = torch.empty((nb * PPB, 4), dtype=torch.int32, device=dev)
    p = P.camera_orbit(-0.15, -0.57, 1500.0, (500.0, 500.0, 40.0), 1920, 1080)
    p.lod_percent, p.enable_frustum_culling = 100, 0

    def chk(ctx, rc, what):
        if rc:
            raise P.PcrError(f"{what} -> {rc}: {ctx.lib.pcr_last_error(ctx.h).decode()}")

    def torch_quantiles(ctx, grid, q):
        """decode_points + one sort by (cell, z) + a gather at the ranks: the planes [len(q), cells] and the counts."""
        ox, oy, cell, w, h = grid
        pts = ctx.decode_points(0, None, out=all_pts)
        x, y = pts[:, 0].to(torch.int64), pts[:, 1].to(torch.int64)
        cx, cy = (x - ox) // cell, (y - oy) // cell
        m = (x >= ox) & (y >= oy) & (cx < w) & (cy < h)
        idx = (cx + cy * w)[m]
        key, _ = torch.sort((idx << 32) | (pts[:, 2].to(torch.int64)[m] + (1 << 31)))
        cnt = torch.bincount(idx, minlength=w * h)
        del x, y, cx, cy, m, idx
        start = torch.cumsum(cnt, 0) - cnt
        occupied = cnt > 0
        planes = torch.full((len(q), w * h), -(1 << 31), dtype=torch.int32, device=dev)
        for j, qj in enumerate(q):
            k = (qj * (cnt[occupied] - 1) + 5000) // 10000
            planes[j, occupied] = ((key[start[occupied] + k] & 0xFFFFFFFF) - (1 << 31)).to(torch.int32)
        torch.cuda.synchronize()
        return planes, cnt.to(torch.int32)

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
            planes = torch.empty((8, cells), dtype=torch.int32, device=dev)
            count = torch.empty(cells, dtype=torch.int32, device=dev)
            top, bottom = torch.empty(cells, dtype=torch.int64, device=dev), torch.empty(cells, dtype=torch.int64, device=dev)
            qst, gst = N.QuantileStats(), N.GridStats()
            r = {}

            def quantiles(q, with_planes=True):
                qa = np.array(q, np.uint32)
                chk(ctx, ctx.lib.pcr_grid_quantiles(ctx.h, 0, -1, C.byref(g), None, None, qa.ctypes.data_as(C.POINTER(N.c_u32)), len(q),
                                                    C.c_void_p(planes.data_ptr()) if with_planes else None, C.c_void_p(count.data_ptr()), flags,
                                                    C.byref(qst)), "pcr_grid_quantiles")

            for tag, q in (("q1", Q1), ("q8", Q8)):
                torch.cuda.synchronize()
                quantiles(q)
                want, want_cnt = torch_quantiles(ctx, grid, q)
                if not torch.equal(planes[:len(q)], want) or not torch.equal(count, want_cnt):
                    sys.exit(f"{name} {label} {tag}: the planes differ from decode_points + sort + gather")
                del want, want_cnt
                t_q = timed(lambda: quantiles(q))
                t0 = time.perf_counter()
                for _ in range(args.torch_reps):
                    torch_quantiles(ctx, grid, q)
                t_alt = (time.perf_counter() - t0) * 1e3 / args.torch_reps
                r[tag] = {"quantiles_ms": round(t_q, 4), "ratio_to_decode_points": round(t_q / t_decode, 3),
                          "decode_plus_torch_sort_host_ms": round(t_alt, 4), "speedup_over_decode_plus_sort": round(t_alt / t_q, 1)}
            t_count = timed(lambda: quantiles(Q1, with_planes=False))
            r["count_only_ms"] = round(t_count, 4)

            def accumulate():
                chk(ctx, ctx.lib.pcr_grid_accumulate(ctx.h, 0, -1, C.byref(g), None, C.c_void_p(top.data_ptr()), C.c_void_p(bottom.data_ptr()),
                                                     C.c_void_p(count.data_ptr()), flags, C.byref(gst)), "pcr_grid_accumulate")

            chk(ctx, ctx.lib.pcr_grid_clear(ctx.h, C.byref(g), C.c_void_p(top.data_ptr()), C.c_void_p(bottom.data_ptr()), C.c_void_p(count.data_ptr())), "pcr_grid_clear")
            r["grid_accumulate_all_ms"] = round(timed(accumulate), 4)
            r["q1_over_count_only"] = round(r["q1"]["quantiles_ms"] / t_count, 3)
            r["q1_over_grid_accumulate_all"] = round(r["q1"]["quantiles_ms"] / r["grid_accumulate_all_ms"], 3)
            # the selection passes of q8 beyond q1's, as a share of the q8 call
            r["q8_minus_q1_share_of_q8"] = round((r["q8"]["quantiles_ms"] - r["q1"]["quantiles_ms"]) / r["q8"]["quantiles_ms"], 3)
            r.update(qst.as_dict())
            r["points_per_occupied_cell"] = round(qst.candidates / max(qst.cells_occupied, 1), 1)
            row[label] = r
            del planes, count, top, bottom
        if row["coarse"]["batches_windowed"] != nb or row["coarse_direct"]["batches_direct"] != nb or row["fine"]["batches_direct"] != nb:
            sys.exit(f"{name}: the grids do not put the batches into the classes this measurement is about: {row}")
        for tag in ("q1", "q8"):
            row[f"windowed_over_direct_{tag}"] = round(row["coarse"][tag]["quantiles_ms"] / row["coarse_direct"][tag]["quantiles_ms"], 3)
        row["windowed_over_direct_count_only"] = round(row["coarse"]["count_only_ms"] / row["coarse_direct"]["count_only_ms"], 3)
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
