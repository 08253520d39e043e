#!/usr/bin/env python3
"""Measurement of pcr_local_moments (pcr_neighbors' plan with k_moments_pairs and k_moments_write in the pair and write kernels'
places) on one GPU -- not the headline bench.

    python tools/bench_moments.py [--points 100000000] [--steps 20] [--warmup 3] [--layouts point_windows,words]
                                  [--radii 128,330,930] [--out profiles/moments.json]

Per layout: the synthetic stream of the headline config, loaded, one frame drawn, then in ONE process on one box, per radius
(lattice steps), `steps` calls between one event pair of each of
  moments_eigen  records, moments and eigen records of every candidate (min_count = 0)
  moments        records and moments
  eigen          records and eigen records (the dense moments are not stored)
  count          all four destinations NULL: everything but the stores of the records and the write
  neighbors_all  pcr_neighbors in mode ALL with N and nn2, beside it: the yardstick -- the same plan, the same pairs, a count and a
                 minimum per pair instead of ten sums
  speedup_over_torch  against what a user has today, on the host clock: decode_points() of everything, voxel keys, a torch sort,
                      27 searchsorted joins of the buckets expanded to pairs piece by piece, ten scatter-adds
Every timed result is first compared with the torch alternative's: records, moments (exact), and the eigen records with
pcr_moments_eigen of the alternative's moments. `pairs_bound` is the call's statistic, `pair_tests_per_s` = pairs_bound /
moments_eigen time, `ratio_to_neighbors` = moments_eigen / neighbors_all. Prints one JSON line and writes it to --out.
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
PAIRS = 1 << 26                    # pairs the torch alternative expands at a time
PRODUCTS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layouts", default="point_windows,words")
    ap.add_argument("--radii", default="128,330,930")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moments.json"))
    args = ap.parse_args()

    import torch
    import pcrhpg24_amd as P
    from pcrhpg24_amd import _native as N
    if not torch.cuda.is_available():
        sys.exit("bench_moments.py measures on the GPU: none found")
    n = args.points
    radii = [int(c) for c in args.radii.split(",")]
    t0 = time.time()
    image, st = P.synth_encode(n, 0x5EED, 0, n, CHUNK, args.threads)
    f = P.HuffmanFile(image)
    nb = f.numBatches
    rec = {"what": "pcr_local_moments over the whole synthetic stream, no clip, min_count = 0, beside pcr_neighbors ALL with N and nn2",
           "kernel_version": P.kernel_version(), "points_in": n, "points_decoded": nb * PPB, "batches": nb, "steps": args.steps, "warmup": args.warmup,
           "generate_s": round(time.time() - t0, 1), "radii": radii, "layouts": {},
           "not_tried": ["the products through 32 x 32 -> 64 multiply-adds or f64 FMAs instead of 24-bit multiplies", "another flush cadence",
                         "the eigen solve in a kernel of its own over the dense moments"]}
    print(f"stream of {nb} batches generated in {rec['generate_s']} s", file=sys.stderr, flush=True)
    dev = torch.device("cuda", 0)
    total = nb * PPB
    all_pts = torch.empty((total, 4), dtype=torch.int32, device=dev)
    p = P.camera_orbit(-0.15, -0.57, 1500.0, (500.0, 500.0, 40.0), 1920, 1080)
    p.lod_percent, p.enable_frustum_culling = 100, 0

    def chk(ctx, rc, what):
        if rc:
            raise P.PcrError(f"{what} -> {rc}: {ctx.lib.pcr_last_error(ctx.h).decode()}")

    def torch_moments(ctx, r):
        """today's way: the whole cloud decoded, sorted by voxel key, the 27 bucket joins expanded to pairs, ten scatter-adds:
        (records, moments int64 [total, 10] by row)"""
        pts = ctx.decode_points(0, None, out=all_pts)
        xyz = pts[:, :3].to(torch.int64)
        v = torch.div(xyz, r, rounding_mode="floor")
        v = v - v.amin(dim=0) + 1
        key = v[:, 0] | (v[:, 1] << 21) | (v[:, 2] << 42)
        del v
        key, order = torch.sort(key)
        xyz = xyz[order]
        vkeys, vlen = torch.unique_consecutive(key, return_counts=True)
        vstart = torch.cumsum(vlen, 0) - vlen
        vid = torch.repeat_interleave(torch.arange(vkeys.shape[0], device=dev), vlen)
        del key
        sums = torch.zeros((10, total), dtype=torch.int64, device=dev)
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    other = vkeys + (dx + (dy << 21) + (dz << 42))
                    at = torch.searchsorted(vkeys, other).clamp_(max=vkeys.shape[0] - 1)
                    hit = vkeys[at] == other
                    first = torch.where(hit, vstart[at], torch.zeros_like(vstart))[vid]
                    cnt = torch.where(hit, vlen[at], torch.zeros_like(vlen))[vid]
                    cum = torch.cumsum(cnt, 0)
                    a, base = 0, 0
                    while a < total:
                        b = max(a + 1, int(torch.searchsorted(cum, torch.tensor(base + PAIRS, device=dev), right=True)))
                        c = cnt[a:b]
                        tot = int(cum[b - 1]) - base
                        if tot:
                            seg = torch.cumsum(c, 0) - c
                            ii = torch.repeat_interleave(torch.arange(a, b, device=dev), c)
                            jj = torch.repeat_interleave(first[a:b] - seg, c) + torch.arange(tot, device=dev)
                            d = xyz[jj] - xyz[ii]                       # neighbour minus centre
                            inside = ((d * d).sum(dim=1) <= r * r).to(torch.int64)
                            d = d * inside[:, None]
                            sums[0].scatter_add_(0, ii, inside)
                            for k in range(3):
                                sums[1 + k].scatter_add_(0, ii, d[:, k])
                            for k, (x, y) in enumerate(PRODUCTS):
                                sums[4 + k].scatter_add_(0, ii, d[:, x] * d[:, y])
                        a, base = b, base + tot
        out = torch.empty((total, 10), dtype=torch.int64, device=dev)
        out[order] = sums.t()
        torch.cuda.synchronize()
        return pts, out

    PIECE = 1 << 24                 # rows per comparison, as tools/bench_denoise.py

    def same(a, b):
        return a.shape == b.shape and all(torch.equal(a[i:i + PIECE], b[i:i + PIECE]) for i in range(0, a.shape[0], PIECE))

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

        row = {"radii": {}}
        ctx.batch_point_bounds()                            # (the exact boxes: once per context, tools/bench_select.py times it)
        for r in radii:
            cnt, nst = C.c_int64(), N.NeighborsStats()
            t0 = time.perf_counter()
            want_pts, want_m = torch_moments(ctx, r)
            t_alt = time.perf_counter() - t0
            want_e = ctx.moments_eigen(want_m)
            out = torch.empty((total, 4), dtype=torch.int32, device=dev)
            mom = torch.empty((total, 10), dtype=torch.int64, device=dev)
            eig = torch.empty((total, 6), dtype=torch.float64, device=dev)
            extra = [torch.empty(total, dtype=torch.int64, device=dev) for _ in range(2)]
            torch.cuda.synchronize()

            def call(points, moments, eigen, cap):
                chk(ctx, ctx.lib.pcr_local_moments(ctx.h, 0, -1, r, None, 0, C.c_void_p(points), None, C.c_void_p(moments), C.c_void_p(eigen), cap,
                                                   C.byref(cnt), C.byref(nst)), "pcr_local_moments")

            def neighbors():
                chk(ctx, ctx.lib.pcr_neighbors(ctx.h, 0, -1, r, None, 0, 0, C.c_void_p(out.data_ptr()), None, C.c_void_p(extra[0].data_ptr()),
                                               C.c_void_p(extra[1].data_ptr()), total, C.byref(cnt), C.byref(nst)), "pcr_neighbors")

            forms = {"moments_eigen": (out.data_ptr(), mom.data_ptr(), eig.data_ptr(), total), "moments": (out.data_ptr(), mom.data_ptr(), None, total),
                     "eigen": (out.data_ptr(), None, eig.data_ptr(), total), "count": (None, None, None, 0)}
            for label, a in forms.items():                  # every timed form is checked first
                mom.zero_(); eig.zero_()
                call(*a)
                ok = cnt.value == total
                if ok and a[0]:
                    ok = same(out, want_pts)
                if ok and a[1]:
                    ok = same(mom, want_m)
                if ok and a[2]:
                    ok = same(eig.view(torch.int64), want_e.view(torch.int64))
                if not ok:
                    sys.exit(f"{name} radius {r} {label}: pcr_local_moments differs from the torch alternative")
            neighbors()
            if not same(extra[0], want_m[:, 0].contiguous()):
                sys.exit(f"{name} radius {r}: pcr_neighbors' N differs from the torch alternative's n")
            call(*forms["moments_eigen"])
            stats = nst.as_dict()
            res = {"voxels": stats["voxels"], "runs": stats["runs"], "table_slots": stats["table_slots"],
                   "points_per_voxel": round(stats["points_considered"] / max(stats["voxels"], 1), 3), "max_voxel_points": stats["max_voxel_points"],
                   "pairs_bound": stats["pairs_bound"]}
            del want_pts, want_m, want_e
            res["neighbors_all_ms"] = round(timed(neighbors), 4)
            for label, a in forms.items():
                res[label + "_ms"] = round(timed(lambda: call(*a)), 4)
            res["neighbors_all_again_ms"] = round(timed(neighbors), 4)
            res["pair_tests_per_s"] = round(stats["pairs_bound"] / (res["moments_eigen_ms"] * 1e-3), 1)
            res["ratio_to_neighbors"] = round(res["moments_eigen_ms"] / res["neighbors_all_ms"], 3)
            res["ratio_to_neighbors_moments_only"] = round(res["moments_ms"] / res["neighbors_all_ms"], 3)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                call(*forms["moments_eigen"])
            host_ms = (time.perf_counter() - t0) * 1e3 / args.steps
            res.update(moments_eigen_host_ms=round(host_ms, 4), decode_plus_torch_host_ms=round(t_alt * 1e3, 2), speedup_over_torch=round(t_alt * 1e3 / host_ms, 2))
            row["radii"][str(r)] = res
            print(f"{name} radius {r}: {res}", file=sys.stderr, flush=True)
            del out, mom, eig, extra
            torch.cuda.empty_cache()
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
