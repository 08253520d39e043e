#!/usr/bin/env python3
"""Measurement of pcr_knn (pcr_neighbors' plan with k_knn_pairs<K> and k_knn_write in the pair and write kernels' places) on one GPU --
not the headline bench.

    python tools/bench_knn.py [--points 10000000] [--steps 10] [--warmup 2] [--layouts point_windows,words]
                              [--radii 128,330,930] [--ks 1,8,16] [--out profiles/knn_1e7.json]

Per layout: the synthetic stream of the headline config, loaded, one frame drawn, then in ONE process on one box, per radius
(lattice steps) and k, `steps` calls between one event pair of each of
  knn            records and the k words of every candidate (min_found = 0)
  keep           records only, min_found = k: the pair loop runs for the keep bit alone, nothing dense is stored
  count          all three destinations NULL
  neighbors_all  pcr_neighbors in mode ALL with N and nn2, beside it: the yardstick -- the same plan, the same pairs, a count and a
                 minimum per pair instead of the sorted insertion
  speedup_over_torch  (k = the largest) against what a user has today, on the host clock: decode_points() of everything, voxel
                      keys, a torch sort, 27 searchsorted joins of the buckets expanded to pairs piece by piece, per piece two
                      sorts for the rank inside a centre and a merge of the first k by topk
Every timed result is first compared with the torch alternative's: records and words (the lists of a smaller k are prefixes of the
largest k's). `pairs_bound` is the call's statistic, `pair_tests_per_s` = pairs_bound / knn time, `ratio_to_neighbors` = knn /
neighbors_all. Prints one JSON line and writes it to --out.
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
NONE = (1 << 63) - 1               # the alternative's "no neighbour" while it merges (every real word is below 2^62)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--layouts", default="point_windows,words")
    ap.add_argument("--radii", default="128,330,930")
    ap.add_argument("--ks", default="1,8,16")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_1e7.json"))
    args = ap.parse_args()

    import torch
    import pcrhpg24_amd as P
    from pcrhpg24_amd import _native as N
    if not torch.cuda.is_available():
        sys.exit("bench_knn.py measures on the GPU: none found")
    n = args.points
    radii = [int(c) for c in args.radii.split(",")]
    ks = sorted(int(c) for c in args.ks.split(","))
    kmax = ks[-1]
    t0 = time.time()
    image, st = P.synth_encode(n, 0x5EED, 0, n, CHUNK, args.threads)
    f = P.HuffmanFile(image)
    nb = f.numBatches
    rec = {"what": "pcr_knn over the whole synthetic stream, no clip, min_found = 0, beside pcr_neighbors ALL with N and nn2",
           "kernel_version": P.kernel_version(), "points_in": n, "points_decoded": nb * PPB, "batches": nb, "steps": args.steps, "warmup": args.warmup,
           "generate_s": round(time.time() - t0, 1), "radii": radii, "ks": ks, "layouts": {},
           "not_tried": ["pruning neighbour voxels by the current k-th distance", "an early exit", "64-bit multiply-adds for d2 instead of 24-bit squares",
                         "a 32-bit key (d2 and a rank inside the tile) with the row looked up at the end", "the entry loop unrolled by hand",
                         "skipping the pair kernel when min_found == 0 and no words are asked for"]}
    print(f"stream of {nb} batches generated in {rec['generate_s']} s", file=sys.stderr, flush=True)
    dev = torch.device("cuda", 0)
    total = nb * PPB
    all_pts = torch.empty((total, 4), dtype=torch.int32, device=dev)
    p = P.camera_orbit(-0.15, -0.57, 1500.0, (500.0, 500.0, 40.0), 1920, 1080)
    p.lod_percent, p.enable_frustum_culling = 100, 0

    def chk(ctx, rc, what):
        if rc:
            raise P.PcrError(f"{what} -> {rc}: {ctx.lib.pcr_last_error(ctx.h).decode()}")

    def torch_knn(ctx, r):
        """today's way: the whole cloud decoded, sorted by voxel key, the 27 bucket joins expanded to pairs, the first kmax words of
        every centre merged piece by piece: (records, words int64 [total, kmax] by row, -1 for none, N by row)"""
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
        best = torch.full((total, kmax), NONE, dtype=torch.int64, device=dev)
        count = torch.zeros(total, dtype=torch.int64, device=dev)
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
                            d = xyz[jj] - xyz[ii]
                            d2 = (d * d).sum(dim=1)
                            inside = d2 <= r * r
                            count.scatter_add_(0, ii, inside.to(torch.int64))
                            use = inside & (ii != jj)               # another row, the same point or not
                            ii, words = ii[use], (d2[use] << 32) | order[jj[use]]
                            if ii.numel():
                                words, o = torch.sort(words)                    # by word, then stably by centre: the rank inside a centre
                                ii, o = torch.sort(ii[o], stable=True)
                                words = words[o]
                                head = torch.ones_like(ii, dtype=torch.bool)
                                head[1:] = ii[1:] != ii[:-1]
                                start = torch.cummax(torch.where(head, torch.arange(ii.numel(), device=dev), torch.zeros_like(ii)), 0)[0]
                                rank = torch.arange(ii.numel(), device=dev) - start
                                keep = rank < kmax
                                fresh = torch.full((b - a, kmax), NONE, dtype=torch.int64, device=dev)
                                fresh[ii[keep] - a, rank[keep]] = words[keep]
                                both = torch.cat([best[a:b], fresh], dim=1)
                                best[a:b] = torch.topk(both, kmax, dim=1, largest=False, sorted=True)[0]
                        a, base = b, base + tot
        out = torch.empty((total, kmax), dtype=torch.int64, device=dev)
        out[order] = torch.where(best == NONE, torch.full_like(best, -1), best)
        n_in = torch.empty(total, dtype=torch.int64, device=dev)
        n_in[order] = count
        torch.cuda.synchronize()
        return pts, out, n_in

    PIECE = 1 << 22                 # rows per comparison

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
            want_pts, want_w, want_n = torch_knn(ctx, r)
            t_alt = time.perf_counter() - t0
            out = torch.empty((total, 4), dtype=torch.int32, device=dev)
            extra = [torch.empty(total, dtype=torch.int64, device=dev) for _ in range(2)]
            torch.cuda.synchronize()

            def neighbors():
                chk(ctx, ctx.lib.pcr_neighbors(ctx.h, 0, -1, r, None, 0, 0, C.c_void_p(out.data_ptr()), None, C.c_void_p(extra[0].data_ptr()),
                                               C.c_void_p(extra[1].data_ptr()), total, C.byref(cnt), C.byref(nst)), "pcr_neighbors")

            neighbors()
            if not same(extra[0], want_n):
                sys.exit(f"{name} radius {r}: pcr_neighbors' N differs from the torch alternative's")
            res = {"neighbors_all_ms": round(timed(neighbors), 4), "decode_plus_torch_host_ms": round(t_alt * 1e3, 2), "k": {}}
            for k in ks:
                words = torch.empty((total, k), dtype=torch.int64, device=dev)
                found_k = (want_w[:, :k] >= 0).sum(dim=1) == k

                def call(points, knn, min_found, cap):
                    chk(ctx, ctx.lib.pcr_knn(ctx.h, 0, -1, k, r, None, min_found, C.c_void_p(points), None, C.c_void_p(knn), cap, C.byref(cnt), C.byref(nst)),
                        "pcr_knn")

                forms = {"knn": (out.data_ptr(), words.data_ptr(), 0, total), "keep": (out.data_ptr(), None, k, total), "count": (None, None, 0, 0)}
                for label, a in forms.items():              # every timed form is checked first
                    out.zero_(); words.zero_()
                    call(*a)
                    if label == "keep":
                        m = int(found_k.sum())
                        ok = cnt.value == m and same(out[:m], want_pts[found_k])
                    else:
                        ok = cnt.value == total and (not a[0] or same(out, want_pts)) and (not a[1] or same(words, want_w[:, :k].contiguous()))
                    if not ok:
                        sys.exit(f"{name} radius {r} k {k} {label}: pcr_knn differs from the torch alternative")
                call(*forms["knn"])
                stats = nst.as_dict()
                res.update(voxels=stats["voxels"], runs=stats["runs"], table_slots=stats["table_slots"],
                           points_per_voxel=round(stats["points_considered"] / max(stats["voxels"], 1), 3), max_voxel_points=stats["max_voxel_points"],
                           pairs_bound=stats["pairs_bound"])
                rk = {label + "_ms": round(timed(lambda: call(*a)), 4) for label, a in forms.items()}
                rk["pair_tests_per_s"] = round(stats["pairs_bound"] / (rk["knn_ms"] * 1e-3), 1)
                rk["ratio_to_neighbors"] = round(rk["knn_ms"] / res["neighbors_all_ms"], 3)
                rk["ratio_to_neighbors_keep_only"] = round(rk["keep_ms"] / res["neighbors_all_ms"], 3)
                if k == kmax:
                    t0 = time.perf_counter()
                    for _ in range(args.steps):
                        call(*forms["knn"])
                    host_ms = (time.perf_counter() - t0) * 1e3 / args.steps
                    rk.update(knn_host_ms=round(host_ms, 4), speedup_over_torch=round(t_alt * 1e3 / host_ms, 2))
                res["k"][str(k)] = rk
                del words
            res["neighbors_all_again_ms"] = round(timed(neighbors), 4)
            row["radii"][str(r)] = res
            print(f"{name} radius {r}: {res}", file=sys.stderr, flush=True)
            del out, extra, want_pts, want_w, want_n
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
