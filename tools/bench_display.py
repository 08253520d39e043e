#!/usr/bin/env python3
"""Measurement of the display resolves (pcr_resolve_*_display: k_resolve_display) on one GPU -- not the headline bench.

    python tools/bench_display.py [--points 100000000] [--steps 20] [--warmup 3] [--sizes 1920x1080,4096x4096]
                                  [--methods basic,hqs,las] [--windows 0,1,4] [--edl-windows 0,2]
                                  [--out profiles/resolve_display.json]

The synthetic stream of the headline config (and, for `las`, its points in generation order as a 10-10-10 cloud), loaded once; per
image size one frame of each method is drawn (overview camera, LOD 100 %, culling on) and then, in ONE process on one box, every
figure is the average of `steps` calls between one pair of HIP events:
  plain       pcr_resolve_basic / _hqs / _las (code this feature does not touch)
  display     pcr_resolve_*_display at window 0, 1 and 4, without EDL and with edl_window 2 (strength 0.0005)
Each row holds its ratio to the plain resolve of its method and to the bound bytes_min / copy rate, the copy rate being the streaming
copy pcr_measure_hbm reports on the same box. bytes_min = every input word read once + 4 B per pixel written: 8 B per pixel of
framebuffer (hqs: + 16 B of RG / BA; las: + 4 B of point colour per drawn pixel) + 4 B. The target the design set itself: at
4096 x 4096, window 4 without EDL, at most 1.5 x the bound (halo re-reads, mostly from L2, and the two LDS passes); at 1080p a
2-Mpixel stencil is launch-bound and has no target. Prints one JSON line and writes it to --out.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHUNK = 6553600                    # points per Morton-sorted chunk = 100 batches, as bench.py builds the headline stream
TARGET = 1.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="1920x1080,4096x4096")
    ap.add_argument("--methods", default="basic,hqs,las")
    ap.add_argument("--windows", default="0,1,4")
    ap.add_argument("--edl-windows", default="0,2")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resolve_display.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import pcrhpg24_amd as P
    if not torch.cuda.is_available():
        sys.exit("bench_display.py measures on the GPU: none found")
    n = args.points
    methods = args.methods.split(",")
    sizes = [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")]
    rec = {"what": "pcr_resolve_*_display against the plain resolves and the copy-rate bound", "kernel": "k_resolve_display",
           "kernel_version": P.kernel_version(), "points_in": n, "steps": args.steps, "warmup": args.warmup,
           "camera": "overview, LOD 100 %, culling on", "target_ratio_to_bound_4096_window4": TARGET, "rows": []}

    contexts = {}
    t0 = time.time()
    if "basic" in methods or "hqs" in methods:
        image, _ = P.synth_encode(n, 0x5EED, 0, n, CHUNK, args.threads)
        f = P.HuffmanFile(image)
        c = P.Context(0)
        c.set_image_size(*sizes[0])
        c.stream_begin(f.header())
        for b0 in range(0, f.numBatches, 100):
            c.upload_batches(b0, [f.blob(b) for b in range(b0, min(b0 + 100, f.numBatches))])
        contexts["huffman"] = c
    if "las" in methods:
        x, y, z, col = P.synth_points(n, 0x5EED, 0, n)
        q = P.las_quantize(x, y, z, col, P.synth_las_info(n, 0x5EED))
        del x, y, z, col
        c = P.Context(0)
        c.set_image_size(*sizes[0])
        c.las_begin(n)
        nb, XB = len(q[0]), type(q[0][0])
        for b0 in range(0, nb, 100):
            b1 = min(nb, b0 + 100)
            c.las_upload(b0, (XB * (b1 - b0)).from_buffer(q[0], b0 * 64), *(a[b0 * 65536:b1 * 65536] for a in q[1:]))
        del q
        contexts["las"] = c
    rec["prepare_s"] = round(time.time() - t0, 1)
    _, copy_gbps = next(iter(contexts.values())).measure_hbm()
    rec["copy_gbps"] = round(copy_gbps, 1)

    def opts(w, e):
        o = P.DisplayOpts()
        o.window, o.edl_window, o.edl_strength = w, e, 0.0005
        return o

    for W, H in sizes:
        p = P.camera_orbit(-0.15, -0.57, 1500.0, (500.0, 500.0, 40.0), W, H)
        p.lod_percent, p.enable_frustum_culling = 100, 1
        for m in methods:
            ctx = contexts["las" if m == "las" else "huffman"]
            if (ctx.width, ctx.height) != (W, H):
                ctx.set_image_size(W, H)
            ctx.clear()
            if m == "basic":
                ctx.render_basic(p)
            elif m == "hqs":
                ctx.render_hqs_depth(p); ctx.render_hqs_color(p)
            else:
                ctx.render_las(p)
            plain = {"basic": ctx.resolve_basic, "hqs": ctx.resolve_hqs, "las": ctx.resolve_las}[m]
            display = {"basic": ctx.resolve_basic_display, "hqs": ctx.resolve_hqs_display, "las": ctx.resolve_las_display}[m]
            drawn = int((ctx.read_framebuffer() != np.uint64(0xFFFFFFFFFFFFFFFF)).sum())
            bytes_min = W * H * ({"basic": 8, "hqs": 24, "las": 8}[m] + 4) + (4 * drawn if m == "las" else 0)
            bound_ms = bytes_min / (copy_gbps * 1e9) * 1e3

            def timed(call):
                for _ in range(args.warmup):
                    call()
                ctx.synchronize()
                ctx.timing_begin()
                for _ in range(args.steps):
                    call()
                return ctx.timing_end() / args.steps

            t_plain = timed(lambda: plain(p))

            def row(call, ms, w=None, e=None):
                r = {"size": [W, H], "method": m, "call": call, "ms": round(ms, 5), "ratio_to_plain": round(ms / t_plain, 3),
                     "drawn_pixels": drawn, "bytes_min": bytes_min, "bound_ms": round(bound_ms, 5), "ratio_to_bound": round(ms / bound_ms, 3)}
                if w is not None:
                    r["window"], r["edl_window"] = w, e
                rec["rows"].append(r)
                return r

            row("plain", t_plain)
            for e in (int(v) for v in args.edl_windows.split(",")):
                for w in (int(v) for v in args.windows.split(",")):
                    o = opts(w, e)
                    r = row("display", timed(lambda: display(p, o)), w, e)
                    if (W, H) == (4096, 4096) and w == 4 and e == 0:
                        r["target_met"] = bool(r["ratio_to_bound"] <= TARGET)
    for c in contexts.values():
        c.close()
    line = json.dumps(rec)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fo:
            json.dump(rec, fo, indent=1)
    print(line)


if __name__ == "__main__":
    main()
