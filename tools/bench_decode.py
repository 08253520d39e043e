#!/usr/bin/env python3
"""Measurement of pcr_decode_points (k_decode_points) on one GPU -- not the headline bench.

    python tools/bench_decode.py [--points 100000000] [--steps 20] [--warmup 3] [--layouts point_windows,words]
                                 [--out profiles/decode_points.json] [--kernel-stats DIR]

Per layout: the synthetic stream of the headline config, loaded, one frame drawn (so the load-time buffers are gone), then
`steps` pcr_decode_points calls of the whole stream into a torch tensor behind `warmup` untimed ones, between one pair of HIP
events (pcr_timing_begin / pcr_timing_end). Beside it, in the same process on the same box:
  (a) pcr_measure_hbm's streaming copy rate (read + written bytes counted) -- and, for the account, torch's fill rate over the
      output tensor (written bytes only),
  (b) the per-launch time of the unchanged HQS depth pass with the same layout forced (pcr_kernel_timing_*, LOD 100 %, cull 0):
      the existing kernel that runs the same decode chain and no colour work.
The bound: a kernel that did the depth pass's decode and then, without any overlap, moved its bytes at the copy rate takes
t_depth + (layout bytes read + 16 B x points written) / copy_rate; the decode has to take at most 1.10 x that.
"layout bytes read" = what the loaded stream occupies on the device after the first frame (pcr_stream_resident_bytes).
Also: pcr_read_points' host rate over 256 batches (PCIe-bound; no target).

Prints one JSON line and writes it to --out. Kernel time from the profiler comes from a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_decode.py --steps 5 --out ''
    python tools/bench_decode.py --kernel-stats DIR --out profiles/decode_points.json      (merges it into the stored record; no GPU)
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
SLACK = 1.10


def kernel_stats(directory: str) -> dict:
    """Average duration per k_decode_points instantiation from rocprofv3's kernel trace (ns columns Start/End_Timestamp)."""
    out = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name", "")
                if "k_decode_points" not in name:
                    continue
                layout = "words" if "ILi0E" in name or "<0" in name else "point_windows"
                out.setdefault(layout, []).append((int(row.get("Grid_Size_X", row.get("Grid_Size", 0)) or 0),
                                                   (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6))
    res = {}
    for k, v in out.items():
        whole = max(g for g, _ in v)                        # the launches over the whole stream (pcr_read_points decodes in pieces)
        ms = [t for g, t in v if g == whole]
        res[k] = {"launches": len(ms), "avg_ms": round(sum(ms) / len(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layouts", default="point_windows,words")
    ap.add_argument("--depth-frames", type=int, default=20)
    ap.add_argument("--hbm-bytes", type=int, default=2 << 30)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_points.json"))
    ap.add_argument("--kernel-stats", metavar="DIR", default=None, help="merge rocprofv3 kernel-trace results into --out and exit (no GPU)")
    args = ap.parse_args()

    if args.kernel_stats:
        rec = json.load(open(args.out))
        ks = kernel_stats(args.kernel_stats)
        for name, row in rec["layouts"].items():
            row["rocprof_kernel"] = ks.get(name, "not measured")
        json.dump(rec, open(args.out, "w"), indent=1)
        print(json.dumps(rec))
        return

    import torch
    import pcrhpg24_amd as P
    if not torch.cuda.is_available():
        sys.exit("bench_decode.py measures on the GPU: none found")
    n = args.points
    t0 = time.time()
    image, st = P.synth_encode(n, 0x5EED, 0, n, CHUNK, args.threads)
    f = P.HuffmanFile(image)
    nb = f.numBatches
    t_gen = time.time() - t0
    rec = {"what": "pcr_decode_points over the whole synthetic stream", "kernel_version": P.kernel_version(), "points_in": n,
           "points_decoded": nb * PPB, "batches": nb, "steps": args.steps, "warmup": args.warmup, "generate_s": round(t_gen, 1),
           "slack": SLACK, "layouts": {}}
    out = torch.empty((nb * PPB, 4), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    # the device's plain fill rate over the same tensor (written bytes only), beside the copy rate: what stores alone can reach
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out.zero_(); torch.cuda.synchronize()
    ev[0].record()
    for _ in range(5):
        out.zero_()
    ev[1].record(); torch.cuda.synchronize()
    rec["fill_gbps"] = round(out.numel() * 4 * 5 / ev[0].elapsed_time(ev[1]) * 1e-6, 1)
    p = P.camera_orbit(-0.15, -0.57, 1500.0, (500.0, 500.0, 40.0), 1920, 1080)
    p.lod_percent, p.enable_frustum_culling = 100, 0
    copy_gbps = None
    for name in args.layouts.split(","):
        ctx = P.Context(0)
        ctx.set_stream_layout({"point_windows": P.Context.LAYOUT_POINT_WINDOWS, "words": P.Context.LAYOUT_WORDS}[name])
        ctx.set_image_size(1920, 1080)
        ctx.stream_begin(f.header())
        for b0 in range(0, nb, 100):
            ctx.upload_batches(b0, [f.blob(b) for b in range(b0, min(b0 + 100, nb))])
        if copy_gbps is None:
            read_gbps, copy_gbps = ctx.measure_hbm(args.hbm_bytes, 5)
            rec["hbm_read_gbps"], rec["hbm_copy_gbps"] = round(read_gbps, 1), round(copy_gbps, 1)
        # (b) the depth pass, this layout's kernel; the first frame also releases the load-time buffers
        ctx.clear(); ctx.render_hqs_depth(p); ctx.synchronize()
        ctx.kernel_timing(1)
        for _ in range(args.depth_frames):
            ctx.clear(); ctx.render_hqs_depth(p)
        t_depth, depth_launches = ctx.kernel_timing_read()
        ctx.kernel_timing(0)
        layout_bytes = ctx.resident_bytes
        alg_bytes = ctx.algorithmic_bytes

        def call():
            rc = ctx.lib.pcr_decode_points(ctx.h, 0, -1, C.c_void_p(out.data_ptr()), nb * PPB)
            if rc:
                raise P.PcrError(f"pcr_decode_points -> {rc}: {ctx.lib.pcr_last_error(ctx.h).decode()}")

        for _ in range(args.warmup):
            call()
        ctx.synchronize()
        ctx.timing_begin()
        for _ in range(args.steps):
            call()
        ms = ctx.timing_end() / args.steps
        written = 16 * nb * PPB
        bound_ms = t_depth + (layout_bytes + written) / (copy_gbps * 1e9) * 1e3
        row = {"ms_per_call": round(ms, 4), "gpoints_per_s": round(nb * PPB / ms * 1e-6, 2),
               "algorithmic_bytes_read": alg_bytes, "layout_bytes_read": layout_bytes, "bytes_written": written,
               "gb_per_s_algorithmic": round((alg_bytes + written) / ms * 1e-6, 1), "gb_per_s_layout": round((layout_bytes + written) / ms * 1e-6, 1),
               "hqs_depth_pass_ms": round(t_depth, 4), "hqs_depth_launches": depth_launches,
               "bound_ms": round(bound_ms, 4), "ratio_to_bound": round(ms / bound_ms, 3), "within_1.10x": bool(ms <= SLACK * bound_ms),
               "rocprof_kernel": "not measured"}
        if name == args.layouts.split(",")[0]:
            k = min(nb, 256)
            t0 = time.time()
            host = ctx.read_points(0, k)
            dt = time.time() - t0
            row["read_points_host"] = {"batches": k, "seconds": round(dt, 3), "gb_per_s": round(host.nbytes / dt * 1e-9, 2)}
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
