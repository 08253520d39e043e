#!/usr/bin/env python3
"""Measurement of pcr_neighbors (k_thin_runs, k_denoise_clear, k_neighbors_count, k_neighbors_alloc, k_neighbors_fill,
k_neighbors_pairs, k_thin_totals, k_neighbors_write) on one GPU -- not the headline bench.

    python tools/bench_neighbors.py [--points 100000000] [--steps 20] [--warmup 3] [--layouts point_windows,words]
                                    [--radii 128,330,930] [--out profiles/neighbors.json]

Per layout: the synthetic stream of the headline config, loaded, one frame drawn, then in ONE process on one box, per radius
(lattice steps), `steps` calls between one event pair of each of
  all_attrs     PCR_NEIGHBORS_ALL with records, N and nn2: every pair of the 27 voxels is tested
  keep_attrs    PCR_NEIGHBORS_KEEP at min_count = the median N, with N and nn2 (no early exit)
  keep          the same without N and nn2: a wave leaves the pair loop once all its centres have min_count -- the early exit's worth
  count         all four destinations NULL, PCR_NEIGHBORS_KEEP: everything but the write, with the early exit
  denoise_keep  pcr_denoise at cell = radius, max_count = min_count - 1, beside it: the same decode passes plus 27 lookups per voxel
                and no pairs
  speedup_over_torch  against what a user has today, on the host clock: decode_points() of everything, voxel keys, a torch sort,
                      27 searchsorted joins of the buckets expanded to pairs piece by piece, scatter reductions
Every timed result is first compared with the torch alternative's: records, rows, N and nn2. `pairs_bound` is the call's
statistic, `pair_tests_per_s` = pairs_bound / all_attrs time: the rate the pair kernel achieves including the index build.
Prints one JSON line and writes it to --out.
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
PAIRS = 1 << 27                    # pairs the torch alternative expands at a time
ALL, KEEP = 0, 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layouts", default="point_windows,words")
    ap.add_argument("--radii", default="128,330,930")
    ap.add_argument("--torch-reps", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neighbors.json"))
    args = ap.parse_args()

    import torch
    import pcrhpg24_amd as P
    from pcrhpg24_amd import _native as N
    if not torch.cuda.is_available():
        sys.exit("bench_neighbors.py measures on the GPU: none found")
    n = args.points
    radii = [int(c) for c in args.radii.split(",")]
    t0 = time.time()
    image, st = P.synth_encode(n, 0x5EED, 0, n, CHUNK, args.threads)
    f = P.HuffmanFile(image)
    nb = f.numBatches
    rec = {"what": "pcr_neighbors over the whole synthetic stream, no clip, min_count = the median N", "kernel_version": P.kernel_version(),
           "points_in": n, "points_decoded": nb * PPB, "batches": nb, "steps": args.steps, "warmup": args.warmup, "generate_s": round(time.time() - t0, 1),
           "radii": radii, "layouts": {},
           "not_tried": ["lanes over the neighbour points instead of the centres for voxels of a few points", "an LDS pre-merge of the insertions"]}
    print(f"stream of {nb} batches generated in {rec['generate_s']} s", file=sys.stderr, flush=True)
    dev = torch.device("cuda", 0)
    total = nb * PPB
    all_pts = torch.empty((total, 4), dtype=torch.int32, device=dev)
    p = P.camera_orbit(-0.15, -0.57, 1500.0, (500.0, 500.0, 40.0), 1920, 1080)
    p.lod_percent, p.enable_frustum_culling = 100, 0
    BIG = (1 << 63) - 1

    def chk(ctx, rc, what):
        if rc:
            raise P.PcrError(f"{what} -> {rc}: {ctx.lib.pcr_last_error(ctx.h).decode()}")

    def torch_neighbors(ctx, r):
        """today's way: the whole cloud decoded, sorted by voxel key, the 27 bucket joins expanded to pairs: (records, N, nn2 as int64)"""
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
        count = torch.zeros(total, dtype=torch.int64, device=dev)
        zeros = torch.zeros(total, dtype=torch.int64, device=dev)
        best = torch.full((total,), BIG, dtype=torch.int64, device=dev)
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
                            d = xyz[ii] - xyz[jj]
                            d2 = (d * d).sum(dim=1)
                            inside = d2 <= r * r
                            count.scatter_add_(0, ii, inside.to(torch.int64))
                            zeros.scatter_add_(0, ii, (d2 == 0).to(torch.int64))
                            best.scatter_reduce_(0, ii, torch.where(inside & (d2 > 0), d2, torch.full_like(d2, BIG)), "amin")
                        a, base = b, base + tot
        nn2 = torch.where(zeros >= 2, torch.zeros_like(best), torch.where(best == BIG, torch.full_like(best, -1), best))
        out_n, out_nn2 = torch.empty_like(count), torch.empty_like(nn2)
        out_n[order] = count
        out_nn2[order] = nn2
        torch.cuda.synchronize()
        return pts, out_n, out_nn2

    PIECE = 1 << 24                 # rows per gather and per comparison, as tools/bench_denoise.py

    def same(a, b):
        return a.shape == b.shape and all(torch.equal(a[i:i + PIECE], b[i:i + PIECE]) for i in range(0, a.shape[0], PIECE))

    def gather(src, rows):
        out = torch.empty((rows.shape[0],) + tuple(src.shape[1:]), dtype=src.dtype, device=dev)
        for i in range(0, rows.shape[0], PIECE):
            out[i:i + PIECE] = src[rows[i:i + PIECE]]
        return out

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
            cnt, nst, dst = C.c_int64(), N.NeighborsStats(), N.DenoiseStats()
            t0 = time.perf_counter()
            want_pts, want_n, want_nn2 = torch_neighbors(ctx, r)
            t_alt = [time.perf_counter() - t0]
            for _ in range(args.torch_reps - 1):
                t0 = time.perf_counter()
                torch_neighbors(ctx, r)
                t_alt.append(time.perf_counter() - t0)
            min_count = int(torch.sort(want_n).values[total // 2])
            keep_rows = torch.nonzero(want_n >= min_count).reshape(-1)
            every = torch.arange(total, device=dev)
            out = torch.empty((total, 4), dtype=torch.int32, device=dev)
            extra = [torch.empty(total, dtype=torch.int64, device=dev) for _ in range(3)]
            torch.cuda.synchronize()

            def call(mode, points, rows, counts, nn2, cap):
                chk(ctx, ctx.lib.pcr_neighbors(ctx.h, 0, -1, r, None, min_count, mode, C.c_void_p(points), C.c_void_p(rows), C.c_void_p(counts),
                                               C.c_void_p(nn2), cap, C.byref(cnt), C.byref(nst)), "pcr_neighbors")

            ptrs = [out.data_ptr()] + [t.data_ptr() for t in extra]
            forms = {"all_attrs": (ALL, ptrs[0], None, ptrs[2], ptrs[3], total), "keep_attrs": (KEEP, ptrs[0], None, ptrs[2], ptrs[3], total),
                     "keep": (KEEP, ptrs[0], None, None, None, total), "count": (KEEP, None, None, None, None, 0)}
            for label, a in forms.items():                  # every timed form is checked first; the rows once, with all four outputs
                rows = every if a[0] == ALL else keep_rows
                call(*a)
                ok = cnt.value == rows.shape[0]
                if ok and a[1]:
                    ok = same(out[:cnt.value], gather(want_pts, rows))
                if ok and a[3]:
                    ok = same(extra[1][:cnt.value], gather(want_n, rows)) and same(extra[2][:cnt.value], gather(want_nn2, rows))
                if not ok:
                    sys.exit(f"{name} radius {r} {label}: pcr_neighbors differs from the torch alternative")
            call(KEEP, *ptrs, total)
            if not same(extra[0][:cnt.value], keep_rows):
                sys.exit(f"{name} radius {r}: the rows differ from the torch alternative")
            stats = nst.as_dict()
            res = {"min_count": min_count, "kept": int(keep_rows.shape[0]), "voxels": stats["voxels"], "runs": stats["runs"], "table_slots": stats["table_slots"],
                   "points_per_voxel": round(stats["points_considered"] / max(stats["voxels"], 1), 3), "max_voxel_points": stats["max_voxel_points"],
                   "pairs_bound": stats["pairs_bound"]}
            del want_pts, want_n, want_nn2, keep_rows, every
            for label, a in forms.items():
                res[label + "_ms"] = round(timed(lambda: call(*a)), 4)
            res["pair_tests_per_s"] = round(stats["pairs_bound"] / (res["all_attrs_ms"] * 1e-3), 1)
            res["early_exit_worth"] = round(res["keep_attrs_ms"] / res["keep_ms"], 3)
            vox = P.as_voxels((0, 0, 0, r))

            def denoise(points, cap):
                chk(ctx, ctx.lib.pcr_denoise(ctx.h, 0, -1, C.byref(vox), None, max(min_count - 1, 0), 0, C.c_void_p(points), None, cap, C.byref(cnt),
                                             C.byref(dst)), "pcr_denoise")

            res["denoise_keep_ms"] = round(timed(lambda: denoise(ptrs[0], total)), 4)
            res["denoise_count_ms"] = round(timed(lambda: denoise(None, 0)), 4)
            res["ratio_to_denoise"] = round(res["keep_ms"] / res["denoise_keep_ms"], 3)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                call(*forms["all_attrs"])
            host_ms = (time.perf_counter() - t0) * 1e3 / args.steps
            res.update(all_attrs_host_ms=round(host_ms, 4), decode_plus_torch_host_ms=round(min(t_alt) * 1e3, 2),
                       speedup_over_torch=round(min(t_alt) * 1e3 / host_ms, 2))
            row["radii"][str(r)] = res
            print(f"{name} radius {r}: {res}", file=sys.stderr, flush=True)
            del out, extra
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
