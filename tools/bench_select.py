#!/usr/bin/env python3
"""Measurement of pcr_select_box (k_point_bounds, k_select_count, k_select_write) on one GPU -- not the headline bench.

    python tools/bench_select.py [--points 100000000] [--steps 20] [--warmup 3] [--layouts point_windows,words]
                                 [--out profiles/select_box.json] [--kernel-stats DIR]

Per layout: the synthetic stream of the headline config, loaded, one frame drawn, then in ONE process on one box
  decode      `steps` pcr_decode_points calls of the whole stream between one pair of HIP events (tools/bench_decode.py's figure)
  bounds      the first pcr_batch_point_bounds call of the context: k_point_bounds over every batch + the read-back
  full        pcr_select_box with the whole int32 range: the first call (classification from the cached boxes), then `steps`
              calls between one event pair -- every batch is inside, so this is the decode path + the call's synchronisation
  1pct/10pct  boxes that select about 1 % and 10 % of the points: `steps` calls into a tensor of exactly the selected size,
              the batch classes, and beside them today's alternative: pcr_decode_points of everything + a torch boolean mask
              on the device (host clock around calls that end in a synchronise), and the model time
              (2 x straddling + inside) / batches x t_decode
  count       a count-only call with a slab box every batch straddles: k_select_count over the whole stream, per batch,
              beside k_point_bounds per batch and the HQS depth pass per batch (pcr_kernel_timing_*, LOD 100 %, cull 0)
Every selection is compared with the masked decode before it is timed. Prints one JSON line and writes it to --out.
Kernel times from the profiler come from a run of their own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_select.py --steps 3 --out ''
    python tools/bench_select.py --kernel-stats DIR --out profiles/select_box.json       (merges into the stored record; no GPU)
A number that was not measured on the GPU is reported as "not measured".
"""
from __future__ import annotations

import argparse
import csv
import ctypes as C
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHUNK = 6553600                    # points per Morton-sorted chunk = 100 batches, as bench.py builds the headline stream
PPB = 65536
I32 = (-(1 << 31), (1 << 31) - 1)
BOXES = {                          # x, y in the tile's millimetres, every z
    "full": ((I32[0],) * 3, (I32[1],) * 3),
    "1pct": ((450_000, 450_000, I32[0]), (550_000, 550_000, I32[1])),
    "10pct": ((300_000, 300_000, I32[0]), (616_228, 616_228, I32[1])),
}
SLAB = ((I32[0],) * 3, (I32[1], I32[1], 30_000))        # cuts through every batch: all straddle
KERNELS = ("k_point_bounds", "k_select_count", "k_select_write", "k_decode_points", "k_render")


def kernel_stats(directory: str) -> dict:
    """Per kernel and template arguments: launches, average milliseconds, average workgroups, microseconds per workgroup."""
    rows = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name", "")
                short = next((k for k in KERNELS if k in name), None)
                if not short:
                    continue
                key = name.split("(")[0].replace("void ", "").replace("pcr::", "")
                grid = int(row.get("Grid_Size_X", row.get("Grid_Size", 0)) or 0)
                wg = int(row.get("Workgroup_Size_X", row.get("Workgroup_Size", 1024)) or 1024)
                rows.setdefault(key, []).append((max(grid // max(wg, 1), 1), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6))
    out = {}
    for key, v in sorted(rows.items()):
        big = max(g for g, _ in v)
        ms = [t for g, t in v if g == big]               # the launches over the most batches
        out[key] = {"launches": len(ms), "workgroups": big, "avg_ms": round(sum(ms) / len(ms), 4), "us_per_workgroup": round(sum(ms) / len(ms) / big * 1e3, 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layouts", default="point_windows,words")
    ap.add_argument("--depth-frames", type=int, default=20)
    ap.add_argument("--mask-reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_box.json"))
    ap.add_argument("--kernel-stats", metavar="DIR", default=None, help="merge rocprofv3 kernel-trace results into --out and exit (no GPU)")
    args = ap.parse_args()

    if args.kernel_stats:
        rec = json.load(open(args.out))
        rec["rocprof_kernels"] = kernel_stats(args.kernel_stats) or "not measured"
        json.dump(rec, open(args.out, "w"), indent=1)
        print(json.dumps(rec))
        return

    import torch
    import pcrhpg24_amd as P
    from pcrhpg24_amd import _native as N
    if not torch.cuda.is_available():
        sys.exit("bench_select.py measures on the GPU: none found")
    n = args.points
    t0 = time.time()
    image, st = P.synth_encode(n, 0x5EED, 0, n, CHUNK, args.threads)
    f = P.HuffmanFile(image)
    nb = f.numBatches
    rec = {"what": "pcr_select_box over the whole synthetic stream", "kernel_version": P.kernel_version(), "points_in": n,
           "points_decoded": nb * PPB, "batches": nb, "steps": args.steps, "warmup": args.warmup, "generate_s": round(time.time() - t0, 1),
           "boxes": {k: [list(v[0]), list(v[1])] for k, v in BOXES.items()}, "layouts": {}, "rocprof_kernels": "not measured"}
    dev = torch.device("cuda", 0)
    all_pts = torch.empty((nb * PPB, 4), dtype=torch.int32, device=dev)
    p = P.camera_orbit(-0.15, -0.57, 1500.0, (500.0, 500.0, 40.0), 1920, 1080)
    p.lod_percent, p.enable_frustum_culling = 100, 0

    def chk(ctx, rc, what):
        if rc:
            raise P.PcrError(f"{what} -> {rc}: {ctx.lib.pcr_last_error(ctx.h).decode()}")

    def mask_of(pts, box):
        lo, hi = (torch.tensor(v, dtype=torch.int32, device=dev) for v in box)
        return ((pts[:, :3] >= lo) & (pts[:, :3] <= hi)).all(dim=1)

    for name in args.layouts.split(","):
        ctx = P.Context(0)
        ctx.set_stream_layout({"point_windows": P.Context.LAYOUT_POINT_WINDOWS, "words": P.Context.LAYOUT_WORDS}[name])
        ctx.set_image_size(1920, 1080)
        ctx.stream_begin(f.header())
        for b0 in range(0, nb, 100):
            ctx.upload_batches(b0, [f.blob(b) for b in range(b0, min(b0 + 100, nb))])
        ctx.clear(); ctx.render_hqs_depth(p); ctx.synchronize()
        ctx.kernel_timing(1)
        for _ in range(args.depth_frames):
            ctx.clear(); ctx.render_hqs_depth(p)
        t_depth, _ = ctx.kernel_timing_read()
        ctx.kernel_timing(0)

        def timed(call):
            for _ in range(args.warmup):
                call()
            ctx.synchronize()
            ctx.timing_begin()
            for _ in range(args.steps):
                call()
            return ctx.timing_end() / args.steps

        t_decode = timed(lambda: chk(ctx, ctx.lib.pcr_decode_points(ctx.h, 0, -1, C.c_void_p(all_pts.data_ptr()), nb * PPB), "pcr_decode_points"))
        row = {"decode_points_ms": round(t_decode, 4), "hqs_depth_pass_ms": round(t_depth, 4), "hqs_depth_us_per_batch": round(t_depth / nb * 1e3, 4)}

        # the exact boxes: one k_point_bounds pass over the stream, once per context
        ctx.timing_begin()
        t0 = time.perf_counter()
        ctx.batch_point_bounds()
        host_ms = (time.perf_counter() - t0) * 1e3
        ms = ctx.timing_end()
        row["point_bounds_first_call"] = {"stream_ms": round(ms, 4), "host_ms": round(host_ms, 4), "us_per_batch": round(ms / nb * 1e3, 4)}
        t0 = time.perf_counter()
        ctx.batch_point_bounds()
        row["point_bounds_cached_call_host_ms"] = round((time.perf_counter() - t0) * 1e3, 4)

        ref = ctx.decode_points(0, None, out=all_pts)
        for label, bx in BOXES.items():
            box = P.as_box(bx)
            cnt, sst = C.c_int64(), N.SelectStats()
            t0 = time.perf_counter()
            chk(ctx, ctx.lib.pcr_select_box(ctx.h, 0, -1, C.byref(box), None, 0, C.byref(cnt), C.byref(sst)), "pcr_select_box")
            first_count_ms = (time.perf_counter() - t0) * 1e3
            k = cnt.value
            out = all_pts if label == "full" else torch.empty((k, 4), dtype=torch.int32, device=dev)
            m = mask_of(ref, bx) if label != "full" else None
            want = ref[m] if m is not None else None
            torch.cuda.synchronize()

            def call():
                chk(ctx, ctx.lib.pcr_select_box(ctx.h, 0, -1, C.byref(box), C.c_void_p(out.data_ptr()), k, C.byref(cnt), C.byref(sst)), "pcr_select_box")

            call()
            if want is not None and not torch.equal(out[:k], want):
                sys.exit(f"{name} {label}: the selection differs from the masked decode")
            del want, m
            t_sel = timed(call)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                call()
            host_ms = (time.perf_counter() - t0) * 1e3 / args.steps
            cls = sst.as_dict()
            model = (2 * cls["batches_straddling"] + cls["batches_inside"]) / nb * t_decode
            r = {"selected": k, "share": round(k / (nb * PPB), 5), **cls, "select_ms": round(t_sel, 4), "select_host_ms": round(host_ms, 4),
                 "count_only_first_call_host_ms": round(first_count_ms, 4), "model_ms": round(model, 4), "ratio_to_model": round(t_sel / model, 3) if model else None}
            if label == "full":
                r["minus_decode_ms"] = round(t_sel - t_decode, 4)
            else:
                # today's alternative: decode everything, mask on the device
                def alt():
                    pts = ctx.decode_points(0, None, out=all_pts)
                    sel = pts[mask_of(pts, bx)]
                    torch.cuda.synchronize()
                    return sel
                alt()
                t0 = time.perf_counter()
                for _ in range(args.mask_reps):
                    alt()
                t_alt = (time.perf_counter() - t0) * 1e3 / args.mask_reps
                r["decode_plus_torch_mask_host_ms"] = round(t_alt, 4)
                r["speedup_over_decode_plus_mask"] = round(t_alt / host_ms, 2)
                r["faster_than_decode_plus_mask"] = bool(host_ms < t_alt)
                ref = ctx.decode_points(0, None, out=all_pts)
            row[label] = r
            del out

        # the count kernel alone: a slab every batch straddles, count only
        box = P.as_box(SLAB)
        cnt, sst = C.c_int64(), N.SelectStats()
        t_cnt = timed(lambda: chk(ctx, ctx.lib.pcr_select_box(ctx.h, 0, -1, C.byref(box), None, 0, C.byref(cnt), C.byref(sst)), "pcr_select_box"))
        row["count_only_slab"] = {"batches_straddling": int(sst.batches_straddling), "selected": cnt.value, "call_ms": round(t_cnt, 4),
                                  "us_per_straddling_batch": round(t_cnt / max(int(sst.batches_straddling), 1) * 1e3, 4)}
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
