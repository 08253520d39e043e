#!/usr/bin/env python3
"""Measurement of pcr_select_visible (k_visible_key, k_visible_dilate, k_visible_index, k_visible_count, k_visible_write) on one
GPU -- not the headline bench.

    python tools/bench_visible.py [--points 100000000] [--steps 20] [--warmup 3] [--layouts point_windows,words]
                                  [--out profiles/select_visible.json]

Per layout: the synthetic stream of the headline config, loaded, one frame drawn, then in ONE process on one box, every figure
the average of `steps` calls between one pair of HIP events:
  depth         pcr_clear + pcr_render_hqs_depth with the same params
  screen_*      pcr_select_screen on the same rect, count-only and with records
  front / surface, radius 0 and 2, count-only and with records (points and hits, 32 B a record; the depth plane is not asked
                for), for the whole image and for a rect of 1 % of its pixels around the centre
  torch_*       the route without the call, on the host clock around a device synchronisation: select_screen of the whole image,
                a sort by (pixel, depth, colour, index), a segmented first (front) / compare with the segment's first depth
                (surface), at radius 0
Expectation, stated before the first run: SURFACE is one decode pass more than pcr_select_screen (the key pass) and FRONT two (key
and index), and a decode pass that scatters per-pixel atomics costs about what the HQS depth pass costs. Each figure is recorded
with expected_ms = the select_screen figure measured beside it + 1 (surface) or 2 (front) depth passes, and its ratio to that.
Before anything is timed every result is compared with the torch route (radius 2: a scatter-min plane and a max-pool dilation in
place of the segment's first depth). Prints one JSON line and writes it to --out. A number that was not measured on the GPU is
reported as "not measured".
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layouts", default="point_windows,words")
    ap.add_argument("--lod", type=int, default=100)
    ap.add_argument("--cull", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_visible.json"))
    args = ap.parse_args()

    import torch
    import pcrhpg24_amd as P
    from pcrhpg24_amd import _native as N
    if not torch.cuda.is_available():
        sys.exit("bench_visible.py measures on the GPU: none found")
    n = args.points
    t0 = time.time()
    image, st = P.synth_encode(n, 0x5EED, 0, n, CHUNK, args.threads)
    f = P.HuffmanFile(image)
    nb = f.numBatches
    W, H = 1920, 1080
    p = P.camera_orbit(-0.15, -0.57, 1500.0, (500.0, 500.0, 40.0), W, H)
    p.lod_percent, p.enable_frustum_culling = args.lod, args.cull
    side = (W * H / 100) ** 0.5
    x0, y0 = int(W / 2 - side / 2), int(H / 2 - side / 2)
    rects = {"whole_image": None, "rect_1pct": (x0, y0, x0 + int(round(side)) - 1, y0 + int(round(side)) - 1)}
    rec = {"what": "pcr_select_visible over the whole synthetic stream", "kernel_version": P.kernel_version(), "points_in": n, "batches": nb,
           "steps": args.steps, "warmup": args.warmup, "generate_s": round(time.time() - t0, 1), "image": [W, H], "lod_percent": args.lod,
           "cull": args.cull, "rect_1pct": list(rects["rect_1pct"]),
           "expectation": "ms ~ select_screen ms + 1 (surface) or 2 (front) x hqs_depth_pass_ms", "layouts": {}}

    def say(text):
        print(f"[bench_visible {time.time() - t0:7.1f} s] {text}", file=sys.stderr, flush=True)
    say(f"stream of {nb} batches generated")

    def chk(ctx, rc, what):
        if rc:
            raise P.PcrError(f"{what} -> {rc}: {ctx.lib.pcr_last_error(ctx.h).decode()}")

    def in_rect(pix, rect):
        if rect is None:
            return torch.ones_like(pix, dtype=torch.bool)
        x, y = pix % W, pix // W
        return (x >= rect[0]) & (x <= rect[2]) & (y >= rect[1]) & (y <= rect[3])

    PIECE = 1 << 24                 # rows per gather of records: one indexing call that returns 1e8 rows came back wrong in places

    def rows(t, idx):
        return torch.cat([t[idx[i:i + PIECE]] for i in range(0, idx.shape[0], PIECE)]) if idx.shape[0] else t[:0]

    def torch_route(ctx, mode):
        """(points, hits) of the whole image at radius 0 by a sort: the route the call replaces."""
        pts, hits = ctx.select_screen(p, None)
        pix, depth = hits[:, 0] & 0xFFFFFFFF, hits[:, 0] >> 32
        inside = pix < W * H                                                   # (the others sort behind every pixel and are dropped)
        order = torch.sort(pts[:, 3], stable=True)[1]                          # (the rows come in index order)
        order = order[torch.sort(torch.where(inside, (pix << 32) | depth, (1 << 63) - 1)[order], stable=True)[1]]
        spix, sdepth, keep = pix[order], depth[order], inside[order]
        head = torch.ones_like(spix, dtype=torch.bool)
        head[1:] = spix[1:] != spix[:-1]
        if mode == "front":
            sel = order[head & keep]
        else:
            first = torch.cummax(torch.where(head, torch.arange(len(spix), device=spix.device), 0), 0)[0]
            w = sdepth.to(torch.int32).view(torch.float32).double()
            sel = order[(w <= w[first] * 1.01) & keep]
        sel = torch.sort(sel)[0]
        return rows(pts, sel), rows(hits, sel)

    def torch_reference(pts, hits, mode, radius, rect):
        """The selected rows of select_screen's arrays by a scatter-min plane and a max-pool dilation."""
        pix, depth = hits[:, 0] & 0xFFFFFFFF, hits[:, 0] >> 32
        inside = pix < W * H
        cpix = torch.clamp(pix, max=W * H - 1)
        plane = torch.full((W * H,), 0xFFFFFFFF, dtype=torch.int64, device=pix.device)
        plane.scatter_reduce_(0, pix[inside], depth[inside], "amin")
        if radius:
            d = -torch.nn.functional.max_pool2d(-plane.double().reshape(1, 1, H, W), 2 * radius + 1, 1, radius)
            plane = d.reshape(-1).to(torch.int64)
        dr = plane[cpix].clamp(max=0x7FFFFFFF).to(torch.int32).view(torch.float32).double()
        sel = inside & in_rect(pix, rect) & (depth.to(torch.int32).view(torch.float32).double() <= dr * 1.01)
        if mode == "front":
            key = torch.full((W * H,), (1 << 63) - 1, dtype=torch.int64, device=pix.device)
            full = (depth << 32) | pts[:, 3].to(torch.int64)
            key.scatter_reduce_(0, pix[inside], full[inside], "amin")
            tied = inside & (full == key[cpix])
            index = torch.full((W * H,), (1 << 63) - 1, dtype=torch.int64, device=pix.device)
            index.scatter_reduce_(0, pix[tied], hits[:, 1][tied], "amin")
            sel = sel & tied & (hits[:, 1] == index[cpix])
        return torch.nonzero(sel).reshape(-1)

    for name in args.layouts.split(","):
        ctx = P.Context(0)
        ctx.set_stream_layout({"point_windows": P.Context.LAYOUT_POINT_WINDOWS, "words": P.Context.LAYOUT_WORDS}[name])
        ctx.set_image_size(W, H)
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

        def depth_pass():
            ctx.clear(); ctx.render_hqs_depth(p)
        t_depth = timed(depth_pass)
        row = {"hqs_depth_pass_ms": round(t_depth, 4)}
        say(f"{name}: loaded, depth pass {t_depth:.3f} ms; comparing with the torch route")

        # every result is what the torch route says it is
        all_pts, all_hits = ctx.select_screen(p, None)
        for mode in ("front", "surface"):
            tp, th = torch_route(ctx, mode)
            gp, gh = ctx.select_visible(p, None, mode, 0)
            if not torch.equal(tp, gp) or not torch.equal(th, gh):
                sys.exit(f"{name}: {mode} at radius 0 differs from the sort route")
            for radius in (0, 2):
                for rname, rect in rects.items():
                    sel = torch_reference(all_pts, all_hits, mode, radius, rect)
                    gp, gh = ctx.select_visible(p, rect, mode, radius)
                    if not torch.equal(rows(all_pts, sel), gp) or not torch.equal(rows(all_hits, sel), gh):
                        sys.exit(f"{name}: {mode} radius {radius} {rname} differs from the torch reference")
            del tp, th, gp, gh
        del all_pts, all_hits

        cnt, sst, vst = C.c_int64(), N.ScreenStats(), N.VisibleStats()
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

        def screen(r, pts, hits, cap):
            chk(ctx, ctx.lib.pcr_select_screen(ctx.h, C.byref(p), C.byref(r) if r is not None else None, ptr(pts), ptr(hits), cap, C.byref(cnt), C.byref(sst)),
                "pcr_select_screen")

        def visible(r, mode, radius, pts, hits, cap):
            chk(ctx, ctx.lib.pcr_select_visible(ctx.h, C.byref(p), C.byref(r) if r is not None else None, mode, radius, ptr(pts), ptr(hits), None, cap,
                                                C.byref(cnt), C.byref(vst)), "pcr_select_visible")

        for rname, rect in rects.items():
            say(f"{name}: results agree; timing {rname}" if rect is None else f"{name}: timing {rname}")
            r = P.as_rect(rect)
            out = {}
            t_scr_count = timed(lambda: screen(r, None, None, 0))
            spts, shits = ctx.select_screen(p, r)
            k = spts.shape[0]
            t_scr = timed(lambda: screen(r, spts, shits, k))
            out["select_screen"] = {"selected": k, "count_only_ms": round(t_scr_count, 4), "ms": round(t_scr, 4)}
            del spts, shits
            for mode, passes in (("front", 2), ("surface", 1)):
                for radius in (0, 2):
                    m = N.VISIBLE_FRONT if mode == "front" else N.VISIBLE_SURFACE
                    t_count = timed(lambda: visible(r, m, radius, None, None, 0))
                    vpts, vhits = ctx.select_visible(p, r, mode, radius)
                    kv = vpts.shape[0]
                    t_rec = timed(lambda: visible(r, m, radius, vpts, vhits, kv))
                    e_count, e_rec = t_scr_count + passes * t_depth, t_scr + passes * t_depth
                    out[f"{mode}_radius_{radius}"] = {**vst.as_dict(), "count_only_ms": round(t_count, 4), "count_only_expected_ms": round(e_count, 4),
                                                      "count_only_ratio": round(t_count / e_count, 3), "ms": round(t_rec, 4), "expected_ms": round(e_rec, 4),
                                                      "ratio": round(t_rec / e_rec, 3), "bytes_written": kv * 32}
                    del vpts, vhits
            row[rname] = out
        for mode in ("front", "surface"):
            times = []
            for _ in range(3):
                torch.cuda.synchronize(); t1 = time.perf_counter()
                tp, th = torch_route(ctx, mode)
                torch.cuda.synchronize(); times.append((time.perf_counter() - t1) * 1e3)
                del tp, th
            row[f"torch_{mode}_whole_image_ms"] = round(min(times), 2)
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
