#!/usr/bin/env python3
"""Measurement of pcr_plane_support (k_plane_support) and pcr_select_slabs (k_slab_count, k_slab_write) on one GPU -- not the
headline bench.

    python tools/bench_plane.py [--points 100000000] [--steps 20] [--warmup 3] [--layouts point_windows,words]
                                [--out profiles/plane_support.json]

Per layout: the synthetic stream of the headline config, loaded, one frame drawn, the exact batch boxes computed, then in ONE
process on one box
  plane_support   1, 64 and 1024 hypotheses drawn by plane_hypotheses from four batches of the stream, tolerance 10 lattice steps:
                  `steps` calls between one pair of HIP events after `warmup` calls, with the statistics of the host plan
  select_slabs    a thin tilted slab (a cross-section of 9 m through the middle of the tile) and an oriented box (three slabs,
                  100 m x 100 m, rotated by 30 degrees, every z: 1 % of the tile), count-only and with records
  beside each     pcr_select_box count-only over the same batches with a box that cuts nearly every batch on z (a colourless
                  decode with the cheapest test), and what a user had before: decode_points() + a torch float64 matmul and
                  compare over all records (in pieces of 2^18 records), respectively an int64 mask, on the host clock
Every timed result is first compared with that route's counts or records. The expectation: a call costs about a colourless decode
of its decoded batches plus 65 536 x hypotheses_listed tests. Prints one JSON line and writes it to --out. A number that was not
measured on the GPU is reported as "not measured".
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
PIECE = 1 << 18                    # records per piece of the torch route: 2 GiB of float64 at 1024 hypotheses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layouts", default="point_windows,words")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane_support.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import pcrhpg24_amd as P
    from pcrhpg24_amd import _native as N
    if not torch.cuda.is_available():
        sys.exit("bench_plane.py measures on the GPU: none found")
    n = args.points
    t0 = time.time()
    image, st = P.synth_encode(n, 0x5EED, 0, n, CHUNK, args.threads)
    f = P.HuffmanFile(image)
    nb = f.numBatches
    info = f.batch_las_info(0)
    rec = {"what": "pcr_plane_support and pcr_select_slabs over the whole synthetic stream", "kernel_version": P.kernel_version(), "points_in": n,
           "points_decoded": nb * PPB, "batches": nb, "steps": args.steps, "warmup": args.warmup, "generate_s": round(time.time() - t0, 1),
           "tolerance_steps": 10, "layouts": {}}
    dev = torch.device("cuda", 0)
    p = P.camera_orbit(-0.15, -0.57, 1500.0, (500.0, 500.0, 40.0), 1920, 1080)
    p.lod_percent, p.enable_frustum_culling = 100, 0
    c30, s30 = math.cos(math.radians(30.0)), math.sin(math.radians(30.0))
    mid = (500.0, 500.0, 40.0)
    selections = {"thin_tilted": [P.slab_from_world(info, mid, (-s30, c30, 0.2), 4.5)],
                  "oriented_box": [P.slab_from_world(info, mid, (c30, s30, 0.0), 50.0), P.slab_from_world(info, mid, (-s30, c30, 0.0), 50.0),
                                   P.Slab((0, 0, 1), I32[0], I32[1])]}

    def chk(ctx, rc, what):
        if rc:
            raise P.PcrError(f"{what} -> {rc}: {ctx.lib.pcr_last_error(ctx.h).decode()}")

    for name in args.layouts.split(","):
        ctx = P.Context(0)
        ctx.set_stream_layout({"point_windows": P.Context.LAYOUT_POINT_WINDOWS, "words": P.Context.LAYOUT_WORDS}[name])
        ctx.set_image_size(1920, 1080)
        ctx.stream_begin(f.header())
        for b0 in range(0, nb, 100):
            ctx.upload_batches(b0, [f.blob(b) for b in range(b0, min(b0 + 100, nb))])
        ctx.clear(); ctx.render_hqs_depth(p); ctx.synchronize()
        bounds = ctx.batch_point_bounds()                                   # the exact boxes: once per context, not part of a call's time

        def timed(call):
            for _ in range(args.warmup):
                call()
            ctx.synchronize()
            ctx.timing_begin()
            for _ in range(args.steps):
                call()
            return ctx.timing_end() / args.steps

        # the box beside every call: all of x and y, z from the median of the batch centres up: it cuts the batches that span the median
        zmid = int(np.median((bounds[:, 2].astype(np.int64) + bounds[:, 5]) // 2))
        box = P.as_box(((I32[0], I32[0], zmid), (I32[1], I32[1], I32[1])))
        cnt, bst = C.c_int64(), N.SelectStats()

        def box_call():
            chk(ctx, ctx.lib.pcr_select_box(ctx.h, 0, -1, C.byref(box), None, 0, C.byref(cnt), C.byref(bst)), "pcr_select_box")

        t_box = timed(box_call)
        row = {"box_count": {**bst.as_dict(), "count_ms": round(t_box, 4)}, "plane_support": {}, "select_slabs": {}}

        rng = np.random.default_rng(0)
        groups = []
        for b in np.sort(rng.choice(nb, size=min(4, nb), replace=False)):
            pts = ctx.read_points(int(b), 1)
            groups.append(np.stack([pts["x"], pts["y"], pts["z"]], axis=1).astype(np.int64))
        normals, d = P.plane_hypotheses(groups, 1024, rng)
        pool = [P.slab_from_plane(nk, int(dk), P.slab_tolerance(nk, 10)) for nk, dk in zip(normals.tolist(), d.tolist())]
        all_pts = ctx.decode_points()

        def torch_support(hyp):
            nrm = torch.tensor([s.normal for s in hyp], dtype=torch.float64, device=dev).T.contiguous()
            lo = torch.tensor([float(s.lo) for s in hyp], dtype=torch.float64, device=dev)
            hi = torch.tensor([float(s.hi) for s in hyp], dtype=torch.float64, device=dev)
            pts = ctx.decode_points(out=all_pts)
            out = torch.zeros(len(hyp), dtype=torch.int64, device=dev)
            for a in range(0, pts.shape[0], PIECE):
                v = pts[a:a + PIECE, :3].to(torch.float64) @ nrm
                out += ((v >= lo) & (v <= hi)).sum(dim=0)
            res = out.cpu().numpy()
            return res

        for k in (1, 64, 1024):
            hyp = P.as_slabs(pool[:k])
            got = ctx.plane_support(hyp)
            t0 = time.perf_counter()
            want = torch_support(pool[:k])
            t_alt = (time.perf_counter() - t0) * 1e3
            if not np.array_equal(got, want):
                sys.exit(f"{name}: plane_support of {k} hypotheses differs from decode_points + matmul")
            t = timed(lambda: ctx.plane_support(hyp))
            t0 = time.perf_counter()
            for _ in range(args.steps):
                ctx.plane_support(hyp)
            host_ms = (time.perf_counter() - t0) * 1e3 / args.steps
            stt = dict(ctx.plane_stats)
            row["plane_support"][str(len(hyp))] = {**stt, "best_support": int(got.max()), "call_ms": round(t, 4), "call_host_ms": round(host_ms, 4),
                                                   "tests": PPB * stt["hypotheses_listed"],
                                                   "ratio_to_box_count": round(t / t_box, 3), "decode_plus_torch_matmul_host_ms": round(t_alt, 4),
                                                   "speedup_over_decode_plus_matmul": round(t_alt / host_ms, 2)}

        for label, slabs in selections.items():
            arr = P.as_slabs(slabs)
            sst = N.SlabStats()

            def slab_call(dst, cap):
                chk(ctx, ctx.lib.pcr_select_slabs(ctx.h, 0, -1, arr, len(arr), None, 0, dst, cap, C.byref(cnt), C.byref(sst)), "pcr_select_slabs")

            def alt():
                pts = ctx.decode_points(out=all_pts)
                keep = torch.ones(pts.shape[0], dtype=torch.bool, device=dev)
                x, y, z = (pts[:, a].to(torch.int64) for a in range(3))
                for s in slabs:
                    v = x * s.normal[0] + y * s.normal[1] + z * s.normal[2]
                    keep &= (v >= s.lo) & (v <= s.hi)
                sel = pts[keep]
                torch.cuda.synchronize()
                return sel

            slab_call(None, 0)
            k = cnt.value
            out = torch.empty((k, 4), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            slab_call(C.c_void_p(out.data_ptr()), k)
            t0 = time.perf_counter()
            want = alt()
            t_alt = (time.perf_counter() - t0) * 1e3
            if not torch.equal(out, want):
                sys.exit(f"{name} {label}: the slab selection differs from decode_points masked by torch")
            del want
            t_count = timed(lambda: slab_call(None, 0))
            t_rec = timed(lambda: slab_call(C.c_void_p(out.data_ptr()), k))
            t0 = time.perf_counter()
            for _ in range(args.steps):
                slab_call(C.c_void_p(out.data_ptr()), k)
            host_ms = (time.perf_counter() - t0) * 1e3 / args.steps
            row["select_slabs"][label] = {"selected": k, "share": round(k / (nb * PPB), 5), **sst.as_dict(), "count_ms": round(t_count, 4),
                                          "records_ms": round(t_rec, 4), "records_host_ms": round(host_ms, 4), "ratio_to_box_count": round(t_count / t_box, 3),
                                          "decode_plus_torch_mask_host_ms": round(t_alt, 4), "speedup_over_decode_plus_mask": round(t_alt / host_ms, 2)}
            del out
        del all_pts
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
