#!/usr/bin/env python3
"""Measurement of pcr_lod_order (pcr_thin's FIRST plan, then k_lod_coarsen / k_lod_mark per level, k_lod_count and k_lod_write or
k_lod_rows) on one GPU -- not the headline bench.

    python tools/bench_lod_order.py [--points 100000000] [--steps 20] [--warmup 3] [--layouts point_windows,words]
                                    [--cells 128,330] [--levels 8] [--out profiles/lod_order.json]
    rocprofv3 --kernel-trace --stats ... -- python tools/bench_lod_order.py --profile-calls 5 --layouts point_windows --cells 128 --out ""

Per layout: the synthetic stream of the headline config, loaded, one frame drawn, then in ONE process on one box, per finest cell,
`steps` calls between one pair of HIP events of each of
    count                  all three destinations NULL: the plan, the hierarchy and the level counts, nothing written
    points / all           level order: the records alone; the records, the rows and the levels
    rows_points / rows_all the same with PCR_LOD_ROW_ORDER
    drop_all               level order without the rest (PCR_LOD_DROP_REST), all three outputs
and beside them, in the same process,
    thin_finest    pcr_thin FIRST at the finest cell, records and rows
    thin_levels    the sum over the levels of pcr_thin FIRST with records and rows at each level's cell: what a user does today
                   on the GPU (the set differences still to come)
    decode         pcr_decode_points of everything
    torch          what a user has today without this library's thinning, on the host clock: decode_points() of everything, then
                   per level voxel keys, torch.unique(return_inverse) and scatter_reduce(amin) of the row, a stable sort by level
The expectation written down before the first run: the hierarchy and the level pass touch table slots only, so the call should
cost about thin_finest's count phase plus one decode with colours and be well under thin_levels; whether level order costs more or
less than row order is not known. The record says what came out ("expectation"). Every timed result is compared with the torch
route's records, rows and levels before it is timed. Prints one JSON line and writes it to --out. --profile-calls N: nothing is
compared or timed, N calls of `all` per cell run and the process ends -- for a kernel trace of its own.
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
    ap.add_argument("--cells", default="128,330")
    ap.add_argument("--levels", type=int, default=8)
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--profile-calls", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lod_order.json"))
    args = ap.parse_args()

    import torch
    import pcrhpg24_amd as P
    from pcrhpg24_amd import _native as N
    if not torch.cuda.is_available():
        sys.exit("bench_lod_order.py measures on the GPU: none found")
    n, L = args.points, args.levels
    cells = [int(c) for c in args.cells.split(",")]
    t0 = time.time()
    image, st = P.synth_encode(n, 0x5EED, 0, n, CHUNK, args.threads)
    f = P.HuffmanFile(image)
    nb = f.numBatches
    rec = {"what": "pcr_lod_order over the whole synthetic stream, no clip, origin (0, 0, 0)", "kernel_version": P.kernel_version(), "points_in": n,
           "points_decoded": nb * PPB, "batches": nb, "steps": args.steps, "warmup": args.warmup, "generate_s": round(time.time() - t0, 1),
           "cells": cells, "levels": L,
           "expected_before_the_run": "all_ms about thin_finest's count phase plus one decode with colours; well under thin_levels_ms; level order against "
                                      "row order unknown",
           "layouts": {}}
    print(f"stream of {nb} batches generated in {rec['generate_s']} s", file=sys.stderr, flush=True)
    dev = torch.device("cuda", 0)
    rows_n = nb * PPB
    all_pts = torch.empty((rows_n, 4), dtype=torch.int32, device=dev)
    p = P.camera_orbit(-0.15, -0.57, 1500.0, (500.0, 500.0, 40.0), 1920, 1080)
    p.lod_percent, p.enable_frustum_culling = 100, 0

    def chk(ctx, rc, what):
        if rc:
            raise P.PcrError(f"{what} -> {rc}: {ctx.lib.pcr_last_error(ctx.h).decode()}")

    def torch_levels(ctx, cell):
        """today's way: the whole cloud decoded, then per level the first row of every voxel, from the finest level up"""
        pts = ctx.decode_points(0, None, out=all_pts)
        d = pts[:, :3].to(torch.int64)
        d = d - d.amin(dim=0) // (cell << (L - 1)) * (cell << (L - 1))         # whole coarsest cells: the lattices stay nested
        row = torch.arange(rows_n, dtype=torch.int64, device=dev)
        level = torch.full((rows_n,), L, dtype=torch.uint8, device=dev)
        for l in range(L - 1, -1, -1):
            v = torch.div(d, cell << (L - 1 - l), rounding_mode="floor")
            key = v[:, 0] | (v[:, 1] << 21) | (v[:, 2] << 42)
            del v
            uniq, inv = torch.unique(key, return_inverse=True)
            del key
            first = torch.full((uniq.shape[0],), (1 << 63) - 1, dtype=torch.int64, device=dev).scatter_reduce(0, inv, row, "amin")
            del inv, uniq
            level[first] = l
            del first
        del d
        order = torch.sort(level, stable=True).indices
        out, lv = torch.empty_like(pts), level[order]
        for i in range(0, rows_n, 1 << 24):                                    # (gathered in pieces: one gather of 1e8 rows came back wrong in its last 2^26)
            out[i:i + (1 << 24)] = pts[order[i:i + (1 << 24)]]
        torch.cuda.synchronize()
        return out, order, lv, level

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
        out = torch.empty((rows_n, 4), dtype=torch.int32, device=dev)
        out_rows = torch.empty(rows_n, dtype=torch.int64, device=dev)
        out_lv = torch.empty(rows_n, dtype=torch.uint8, device=dev)
        for cell in cells:
            lod = P.as_lod((0, 0, 0, cell, L))
            cnt, lst = C.c_int64(), N.LodStats()

            def call(flags=0, points=None, rows=None, lvs=None, cap=0):
                chk(ctx, ctx.lib.pcr_lod_order(ctx.h, 0, -1, C.byref(lod), None, flags, C.c_void_p(points), C.c_void_p(rows), C.c_void_p(lvs), cap, C.byref(cnt),
                                               C.byref(lst)), "pcr_lod_order")

            def thin(c, points=None, rows=None, cap=0):
                vox = P.as_voxels((0, 0, 0, c))
                chk(ctx, ctx.lib.pcr_thin(ctx.h, 0, -1, C.byref(vox), None, N.THIN_FIRST, C.c_void_p(points), C.c_void_p(rows), cap, C.byref(cnt), None), "pcr_thin")

            po, ro, lo = out.data_ptr(), out_rows.data_ptr(), out_lv.data_ptr()
            if args.profile_calls:
                for _ in range(args.profile_calls):
                    call(0, po, ro, lo, rows_n)
                ctx.synchronize()
                continue
            want, want_rows, want_lv, dense = torch_levels(ctx, cell)
            call(0, po, ro, lo, rows_n)
            if cnt.value != rows_n or not torch.equal(out, want) or not torch.equal(out_rows, want_rows) or not torch.equal(out_lv, want_lv):
                where = {k: int((a != b).reshape(len(a), -1).any(dim=1).nonzero()[:1].sum()) if not torch.equal(a, b) else None
                         for k, a, b in (("points", out, want), ("rows", out_rows, want_rows), ("levels", out_lv, want_lv))}
                sys.exit(f"{name} cell {cell}: pcr_lod_order differs from the torch alternative in level order: count {cnt.value} of {rows_n}, level counts "
                         f"{lst.as_dict()['level_count'][:L + 1]} against {torch.bincount(want_lv.to(torch.int64), minlength=L + 1).tolist()}, first difference at {where}"
                         + (f": row {int(out_rows[where['points']])} is {out[where['points']].tolist()}, expected {want[where['points']].tolist()}, decode_points has "
                            f"{all_pts[int(want_rows[where['points']])].tolist()}; {int((out != want).any(dim=1).sum())} records differ" if where["points"] is not None else ""))
            call(N.LOD_ROW_ORDER, po, ro, lo, rows_n)
            if cnt.value != rows_n or not torch.equal(out, all_pts) or not torch.equal(out_lv, dense) or not torch.equal(out_rows, torch.arange(rows_n, device=dev)):
                sys.exit(f"{name} cell {cell}: pcr_lod_order differs from the torch alternative in row order")
            call(N.LOD_DROP_REST, po, ro, lo, rows_n)
            k = cnt.value
            # (the rest is the last class of the level order: what is kept is a prefix)
            if k != int((want_lv < L).sum()) or not torch.equal(out[:k], want[:k]) or not torch.equal(out_rows[:k], want_rows[:k]) or not torch.equal(out_lv[:k], want_lv[:k]):
                sys.exit(f"{name} cell {cell}: pcr_lod_order differs from the torch alternative without the rest")
            del want, want_rows, want_lv, dense
            stats = lst.as_dict()
            r = {"level_count": stats["level_count"][:L + 1], "runs": stats["runs"], "table_slots": stats["table_slots"],
                 "runs_per_point": round(stats["runs"] / max(stats["points_considered"], 1), 4)}
            r["count_ms"] = round(timed(lambda: call()), 4)
            r["points_ms"] = round(timed(lambda: call(0, po, None, None, rows_n)), 4)
            r["all_ms"] = round(timed(lambda: call(0, po, ro, lo, rows_n)), 4)
            r["rows_points_ms"] = round(timed(lambda: call(N.LOD_ROW_ORDER, po, None, None, rows_n)), 4)
            r["rows_all_ms"] = round(timed(lambda: call(N.LOD_ROW_ORDER, po, ro, lo, rows_n)), 4)
            r["drop_all_ms"] = round(timed(lambda: call(N.LOD_DROP_REST, po, ro, lo, rows_n)), 4)
            r["thin_finest_count_ms"] = round(timed(lambda: thin(cell)), 4)
            r["thin_finest_ms"] = round(timed(lambda: thin(cell, po, ro, rows_n)), 4)
            per_level = [round(timed(lambda c=cell << (L - 1 - l): thin(c, po, ro, rows_n)), 4) for l in range(L)]
            r["thin_per_level_ms"] = per_level
            r["thin_levels_ms"] = round(sum(per_level), 4)
            r["decode_ms"] = round(timed(lambda: ctx.decode_points(0, None, out=all_pts)), 4)
            r["ratio_to_thin_levels"] = round(r["all_ms"] / r["thin_levels_ms"], 3)
            r["over_thin_count_plus_decode"] = round(r["points_ms"] / (r["thin_finest_count_ms"] + r["decode_ms"]), 3)
            r["level_over_row_order"] = round(r["all_ms"] / r["rows_all_ms"], 3)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                call(0, po, ro, lo, rows_n)
            host_ms = (time.perf_counter() - t0) * 1e3 / args.steps
            t0 = time.perf_counter()
            for _ in range(args.torch_reps):
                torch_levels(ctx, cell)
            t_alt = (time.perf_counter() - t0) * 1e3 / args.torch_reps
            r.update(all_host_ms=round(host_ms, 4), decode_plus_torch_host_ms=round(t_alt, 4), speedup_over_torch=round(t_alt / host_ms, 2))
            row["cells"][str(cell)] = r
            print(f"{name} cell {cell}: {r}", file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
        del out, out_rows, out_lv
        torch.cuda.empty_cache()
        rec["layouts"][name] = row
        ctx.close()
    if args.profile_calls:
        return
    line = json.dumps(rec)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fo:
            json.dump(rec, fo, indent=1)
    print(line)


if __name__ == "__main__":
    main()
