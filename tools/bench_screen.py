#!/usr/bin/env python3
"""Measurement of pcr_select_screen / pcr_pick (k_screen_lod, k_screen_count, k_screen_write, k_pick, k_pick_fetch) on one GPU --
not the headline bench.

    python tools/bench_screen.py [--points 100000000] [--steps 20] [--warmup 3] [--layouts point_windows,words]
                                 [--out profiles/select_screen.json]

Per layout: the synthetic stream of the headline config, loaded, one frame drawn, then in ONE process on one box, every figure
the average of `steps` calls between one pair of HIP events:
  depth       pcr_clear + pcr_render_hqs_depth with the same params (and the kernel alone, pcr_kernel_timing_*)
  count       a count-only pcr_select_screen of the whole image: k_screen_lod + k_screen_count + two read-backs. The count pass
              does a depth pass's decode and projection without the scatter, so its yardstick is the depth pass
  whole       pcr_select_screen of the whole image into tensors of exactly the selected size (points and hits: 32 B per point)
  1pct        a rect of 1 % of the image's pixels around its centre
  pick0/pick8 pcr_pick at the image's centre, radius 0 and 8
The bound of a writing call is t_depth_pass + bytes_written / measured copy rate (pcr_measure_hbm); the record holds the ratio of
every figure to its bound, and beside it the ratio pcr_decode_points achieves against its own bound if profiles/decode_points.json
is there. The whole-image selection is compared with pcr_decode_points of the stream before anything is timed: points ==
decoded[index]. Prints one JSON line and writes it to --out. A number that was not measured on the GPU is reported as
"not measured".
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
    ap.add_argument("--lod", type=int, default=100)
    ap.add_argument("--cull", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_screen.json"))
    args = ap.parse_args()

    import torch
    import pcrhpg24_amd as P
    from pcrhpg24_amd import _native as N
    if not torch.cuda.is_available():
        sys.exit("bench_screen.py measures on the GPU: none found")
    n = args.points
    t0 = time.time()
    image, st = P.synth_encode(n, 0x5EED, 0, n, CHUNK, args.threads)
    f = P.HuffmanFile(image)
    nb = f.numBatches
    W, H = 1920, 1080
    p = P.camera_orbit(-0.15, -0.57, 1500.0, (500.0, 500.0, 40.0), W, H)
    p.lod_percent, p.enable_frustum_culling = args.lod, args.cull
    side = (W * H / 100) ** 0.5
    rect_1pct = (int(W / 2 - side / 2), int(H / 2 - side / 2), int(W / 2 - side / 2) + int(round(side)) - 1, int(H / 2 - side / 2) + int(round(side)) - 1)
    rec = {"what": "pcr_select_screen / pcr_pick over the whole synthetic stream", "kernel_version": P.kernel_version(), "points_in": n,
           "batches": nb, "steps": args.steps, "warmup": args.warmup, "generate_s": round(time.time() - t0, 1), "image": [W, H],
           "lod_percent": args.lod, "cull": args.cull, "rect_1pct": list(rect_1pct), "layouts": {}}
    try:
        stored = json.load(open(os.path.join(ROOT, "profiles", "decode_points.json")))
        rec["decode_points_record"] = {"kernel_version": stored["kernel_version"],
                                       "ratio_to_bound": {k: v["ratio_to_bound"] for k, v in stored["layouts"].items()}}
    except (OSError, ValueError, KeyError):
        rec["decode_points_record"] = "not measured"
    dev = torch.device("cuda", 0)

    def chk(ctx, rc, what):
        if rc:
            raise P.PcrError(f"{what} -> {rc}: {ctx.lib.pcr_last_error(ctx.h).decode()}")

    for name in args.layouts.split(","):
        ctx = P.Context(0)
        ctx.set_stream_layout({"point_windows": P.Context.LAYOUT_POINT_WINDOWS, "words": P.Context.LAYOUT_WORDS}[name])
        ctx.set_image_size(W, H)
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

        def depth():
            ctx.clear(); ctx.render_hqs_depth(p)
        ctx.kernel_timing(1)
        t_depth = timed(depth)
        t_depth_kernel, _ = ctx.kernel_timing_read()
        ctx.kernel_timing(0)
        row = {"hqs_depth_pass_ms": round(t_depth, 4), "hqs_depth_kernel_ms": round(t_depth_kernel, 4), "copy_gbps": round(copy_gbps, 1)}

        cnt, sst = C.c_int64(), N.ScreenStats()

        def select(rect, pts, hits, cap):
            rp = C.byref(rect) if rect is not None else None
            chk(ctx, ctx.lib.pcr_select_screen(ctx.h, C.byref(p), rp, C.c_void_p(pts.data_ptr()) if pts is not None else None,
                                               C.c_void_p(hits.data_ptr()) if hits is not None else None, cap, C.byref(cnt), C.byref(sst)), "pcr_select_screen")

        # the selection is what the decode says it is
        pts, hits = ctx.select_screen(p, None)
        decoded = ctx.decode_points(0, None)
        if not torch.equal(pts, decoded[hits[:, 1]]) or not bool((hits[1:, 1] > hits[:-1, 1]).all()):
            sys.exit(f"{name}: the whole-image selection differs from decode_points()[index]")
        del decoded
        k = pts.shape[0]
        t_count = timed(lambda: select(None, None, None, 0))
        row["count_only"] = {"ms": round(t_count, 4), "ratio_to_depth_pass": round(t_count / t_depth, 3), **sst.as_dict()}

        def bound(records):
            return t_depth + records * 32 / (copy_gbps * 1e9) * 1e3

        t_whole = timed(lambda: select(None, pts, hits, k))
        row["whole_image"] = {"selected": k, "ms": round(t_whole, 4), "bytes_written": k * 32, "bound_ms": round(bound(k), 4),
                              "ratio_to_bound": round(t_whole / bound(k), 3)}
        del pts, hits
        r = P.as_rect(rect_1pct)
        spts, shits = ctx.select_screen(p, r)
        k1 = spts.shape[0]
        t_rect = timed(lambda: select(r, spts, shits, k1))
        row["rect_1pct"] = {"selected": k1, "ms": round(t_rect, 4), "bytes_written": k1 * 32, "bound_ms": round(bound(k1), 4),
                            "ratio_to_bound": round(t_rect / bound(k1), 3)}
        for radius in (0, 8):
            pt, hit, found = N.Point(), N.ScreenHit(), C.c_int()
            t_pick = timed(lambda: chk(ctx, ctx.lib.pcr_pick(ctx.h, C.byref(p), W // 2, H // 2, radius, C.byref(pt), C.byref(hit), C.byref(found)), "pcr_pick"))
            row[f"pick_radius_{radius}"] = {"found": bool(found.value), "ms": round(t_pick, 4), "ratio_to_depth_pass": round(t_pick / t_depth, 3)}
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
