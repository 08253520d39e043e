#!/usr/bin/env python3
"""Measurement of pcr_select_polygon (k_polygon_count, k_polygon_write) on one GPU -- not the headline bench.

    python tools/bench_polygon.py [--points 100000000] [--steps 20] [--warmup 3] [--layouts point_windows,words]
                                  [--mask-reps 2] [--out profiles/select_polygon.json]

Per layout: the synthetic stream of the headline config, loaded, one frame drawn, the exact batch boxes computed, then in ONE
process on one box, for each of three polygons (every z)
  strip    a cross-section: a rectangle of 1.3 km x 9 m rotated by 30 degrees through the middle of the tile, about 1 % of the points
  gon64    a regular 64-gon around the middle with the area of a tenth of the tile, about 10 % of the points
  zigzag   a ring of 4096 vertices around the middle whose radius alternates between 330 m and 370 m
    count       `steps` count-only calls between one pair of HIP events
    records     `steps` calls into a tensor of exactly the selected size, the batch classes, edges_listed and edges_max
    box         beside them pcr_select_box of the polygon's bounding box, count-only and records: what decodes no edge
    box + mask  what a user had before: that box selection followed by a torch point-in-polygon mask over its output on the
                device, one int64 pass over the box's records per edge (host clock around calls that end in a synchronise)
Every timed result is first compared with the alternative's records. Reported per polygon: the ratio of the polygon call to
pcr_select_box of the bounding box (the polygon call decodes fewer batches whole and writes fewer records, but every tested point
pays for its batch's edges), count-only and records, and the ratio to the box + mask alternative. Prints one JSON line and writes
it to --out. A number that was not measured on the GPU is reported as "not measured".
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHUNK = 6553600                    # points per Morton-sorted chunk = 100 batches, as bench.py builds the headline stream
PPB = 65536
I32 = (-(1 << 31), (1 << 31) - 1)
MID = (500_000, 500_000)           # the middle of the tile, millimetres


def polygons():
    c, s = math.cos(math.radians(30.0)), math.sin(math.radians(30.0))
    strip = [(round(MID[0] + u * c - v * s), round(MID[1] + u * s + v * c)) for u, v in ((-650_000, -4_500), (650_000, -4_500), (650_000, 4_500), (-650_000, 4_500))]
    r = math.sqrt(0.1e12 / (32.0 * math.sin(2.0 * math.pi / 64.0)))        # area of a regular 64-gon: 32 r^2 sin(2 pi / 64)
    gon = [(round(MID[0] + r * math.cos(2.0 * math.pi * k / 64)), round(MID[1] + r * math.sin(2.0 * math.pi * k / 64))) for k in range(64)]
    zig = [(round(MID[0] + (330_000 if k % 2 == 0 else 370_000) * math.cos(2.0 * math.pi * k / 4096)),
            round(MID[1] + (330_000 if k % 2 == 0 else 370_000) * math.sin(2.0 * math.pi * k / 4096))) for k in range(4096)]
    return {"strip": strip, "gon64": gon, "zigzag": zig}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layouts", default="point_windows,words")
    ap.add_argument("--mask-reps", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_polygon.json"))
    args = ap.parse_args()

    import torch
    import pcrhpg24_amd as P
    from pcrhpg24_amd import _native as N
    if not torch.cuda.is_available():
        sys.exit("bench_polygon.py measures on the GPU: none found")
    n = args.points
    t0 = time.time()
    image, st = P.synth_encode(n, 0x5EED, 0, n, CHUNK, args.threads)
    f = P.HuffmanFile(image)
    nb = f.numBatches
    rings = polygons()
    rec = {"what": "pcr_select_polygon over the whole synthetic stream", "kernel_version": P.kernel_version(), "points_in": n,
           "points_decoded": nb * PPB, "batches": nb, "steps": args.steps, "warmup": args.warmup, "mask_reps": args.mask_reps,
           "generate_s": round(time.time() - t0, 1), "vertices": {k: len(v) for k, v in rings.items()}, "layouts": {}}
    dev = torch.device("cuda", 0)
    p = P.camera_orbit(-0.15, -0.57, 1500.0, (500.0, 500.0, 40.0), 1920, 1080)
    p.lod_percent, p.enable_frustum_culling = 100, 0

    def chk(ctx, rc, what):
        if rc:
            raise P.PcrError(f"{what} -> {rc}: {ctx.lib.pcr_last_error(ctx.h).decode()}")

    def torch_in_poly(pts, ring):
        """The even-odd rule of include/pcr_types.h over the records of a box selection, an int64 pass per edge."""
        x, y = pts[:, 0].to(torch.int64), pts[:, 1].to(torch.int64)
        odd = torch.zeros(len(pts), dtype=torch.bool, device=dev)
        for i, a in enumerate(ring):
            b = ring[(i + 1) % len(ring)]
            if a[1] == b[1]:
                continue
            lo, up = (a, b) if a[1] < b[1] else (b, a)
            odd ^= (y >= lo[1]) & (y < up[1]) & ((x - lo[0]) * (up[1] - lo[1]) < (y - lo[1]) * (up[0] - lo[0]))
        return odd

    for name in args.layouts.split(","):
        ctx = P.Context(0)
        ctx.set_stream_layout({"point_windows": P.Context.LAYOUT_POINT_WINDOWS, "words": P.Context.LAYOUT_WORDS}[name])
        ctx.set_image_size(1920, 1080)
        ctx.stream_begin(f.header())
        for b0 in range(0, nb, 100):
            ctx.upload_batches(b0, [f.blob(b) for b in range(b0, min(b0 + 100, nb))])
        ctx.clear(); ctx.render_hqs_depth(p); ctx.synchronize()
        ctx.batch_point_bounds()                                            # the exact boxes: once per context, not part of a call's time

        def timed(call):
            for _ in range(args.warmup):
                call()
            ctx.synchronize()
            ctx.timing_begin()
            for _ in range(args.steps):
                call()
            return ctx.timing_end() / args.steps

        row = {}
        for label, ring in rings.items():
            poly = P.Polygon(ring)
            xs, ys = [v[0] for v in ring], [v[1] for v in ring]
            box = P.as_box(((min(xs), min(ys), I32[0]), (max(xs), max(ys), I32[1])))
            cnt, pst, bst = C.c_int64(), N.PolygonStats(), N.SelectStats()

            def poly_call(dst, cap):
                chk(ctx, ctx.lib.pcr_select_polygon(ctx.h, 0, -1, C.byref(poly.c), dst, cap, C.byref(cnt), C.byref(pst)), "pcr_select_polygon")

            def box_call(dst, cap):
                chk(ctx, ctx.lib.pcr_select_box(ctx.h, 0, -1, C.byref(box), dst, cap, C.byref(cnt), C.byref(bst)), "pcr_select_box")

            poly_call(None, 0)
            k = cnt.value
            box_call(None, 0)
            kb = cnt.value
            out = torch.empty((k, 4), dtype=torch.int32, device=dev)
            boxed = torch.empty((kb, 4), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()

            def alt():
                box_call(C.c_void_p(boxed.data_ptr()), kb)
                sel = boxed[torch_in_poly(boxed, ring)]
                torch.cuda.synchronize()
                return sel

            poly_call(C.c_void_p(out.data_ptr()), k)
            t0 = time.perf_counter()
            want = alt()
            first_alt_ms = (time.perf_counter() - t0) * 1e3
            if not torch.equal(out, want):
                sys.exit(f"{name} {label}: the polygon selection differs from the box selection masked by torch")
            del want
            t_count = timed(lambda: poly_call(None, 0))
            t_rec = timed(lambda: poly_call(C.c_void_p(out.data_ptr()), k))
            t0 = time.perf_counter()
            for _ in range(args.steps):
                poly_call(C.c_void_p(out.data_ptr()), k)
            host_ms = (time.perf_counter() - t0) * 1e3 / args.steps
            t_box_count = timed(lambda: box_call(None, 0))
            t_box_rec = timed(lambda: box_call(C.c_void_p(boxed.data_ptr()), kb))
            t0 = time.perf_counter()
            for _ in range(args.mask_reps):
                alt()
            t_alt = (time.perf_counter() - t0) * 1e3 / max(args.mask_reps, 1) if args.mask_reps else first_alt_ms
            row[label] = {"selected": k, "share": round(k / (nb * PPB), 5), **pst.as_dict(), "count_ms": round(t_count, 4), "records_ms": round(t_rec, 4),
                          "records_host_ms": round(host_ms, 4),
                          "box": {"selected": kb, **bst.as_dict(), "count_ms": round(t_box_count, 4), "records_ms": round(t_box_rec, 4)},
                          "ratio_to_box_count": round(t_count / t_box_count, 3), "ratio_to_box_records": round(t_rec / t_box_rec, 3),
                          "box_plus_torch_mask_host_ms": round(t_alt, 4), "box_plus_torch_mask_first_call_host_ms": round(first_alt_ms, 4),
                          "speedup_over_box_plus_mask": round(t_alt / host_ms, 2)}
            del out, boxed
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
