#!/usr/bin/env python3
"""Measurement of pcr_components (k_thin_runs, k_denoise_clear, k_components_clear, k_components_count, k_components_link,
k_components_flatten, k_components_verdict, k_denoise_flag, k_thin_totals, k_thin_write, k_components_labels) on one GPU -- not the
headline bench.

    python tools/bench_components.py [--points 100000000] [--steps 20] [--warmup 3] [--layouts point_windows,words]
                                     [--cells 128,330,930] [--out profiles/components.json]

Per layout: the synthetic stream of the headline config, loaded, one frame drawn, then in ONE process on one box, per cell and
connectivity (6, 26):
  min_points  the median of the component size over all points (the upper one), from the torch labelling below
  PCR_COMPONENTS_KEEP, `steps` calls between one event pair of each of
      count   all three destinations NULL: everything but the writes
      points  the records into a tensor of exactly their number
      labels  the records, their rows and their labels
  denoise     pcr_denoise PCR_DENOISE_KEEP at the same cell with a max_count no voxel reaches, so that every voxel pays all 26
              lookups, the same three figures (without labels), measured beside it: the same three decode passes, 26 lookups per
              voxel where the link phase makes 13 (or 3) and a union each; `ratio_to_denoise` = the call's figure / pcr_denoise's
  speedup_over_torch  against what a user has today, on the host clock: decode_points() of everything, voxel keys, torch.unique,
                      the edges by searchsorted, labels by hooking and pointer jumping with scatter_reduce, a gather
Every result, both modes, is compared with the torch alternative's records, rows and labels before anything is timed. Where the
time goes: `link_ms` = count minus pcr_denoise's count (the union-find with its flatten and verdict scans against the 26-lookup
verdict scan; the decode passes are the same), `labels_pass_ms` = labels minus points less the rows.
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
NEVER = 1 << 40                    # a max_count no voxel's 27 cells reach


def forward_offsets(conn):
    """half of the neighbourhood as key differences: every undirected edge once"""
    return [dx + (dy << 21) + (dz << 42) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if (dz, dy, dx) > (0, 0, 0) and (conn == 26 or abs(dx) + abs(dy) + abs(dz) == 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layouts", default="point_windows,words")
    ap.add_argument("--cells", default="128,330,930")
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components.json"))
    args = ap.parse_args()

    import torch
    import pcrhpg24_amd as P
    from pcrhpg24_amd import _native as N
    if not torch.cuda.is_available():
        sys.exit("bench_components.py measures on the GPU: none found")
    n = args.points
    cells = [int(c) for c in args.cells.split(",")]
    t0 = time.time()
    image, st = P.synth_encode(n, 0x5EED, 0, n, CHUNK, args.threads)
    f = P.HuffmanFile(image)
    nb = f.numBatches
    rec = {"what": "pcr_components over the whole synthetic stream, no clip, origin (0, 0, 0), min_points = the median component size over the points",
           "kernel_version": P.kernel_version(), "points_in": n, "points_decoded": nb * PPB, "batches": nb, "steps": args.steps, "warmup": args.warmup,
           "generate_s": round(time.time() - t0, 1), "cells": cells, "layouts": {}}
    print(f"stream of {nb} batches generated in {rec['generate_s']} s", file=sys.stderr, flush=True)
    dev = torch.device("cuda", 0)
    all_pts = torch.empty((nb * PPB, 4), dtype=torch.int32, device=dev)
    p = P.camera_orbit(-0.15, -0.57, 1500.0, (500.0, 500.0, 40.0), 1920, 1080)
    p.lod_percent, p.enable_frustum_culling = 100, 0

    def chk(ctx, rc, what):
        if rc:
            raise P.PcrError(f"{what} -> {rc}: {ctx.lib.pcr_last_error(ctx.h).decode()}")

    def torch_label(ctx, cell, conn):
        """today's way: the whole cloud decoded, the voxels by sorting 64-bit keys, the edges by searchsorted, then hooking by
        minimum and pointer jumping over the voxels ranked by their least row. Per point: (label, size of its component)."""
        pts = ctx.decode_points(0, None, out=all_pts)
        v = torch.div(pts[:, :3].to(torch.int64), cell, rounding_mode="floor")
        v = v - v.amin(dim=0) + 1
        key = v[:, 0] | (v[:, 1] << 21) | (v[:, 2] << 42)
        del v
        uniq, inv, own = torch.unique(key, return_inverse=True, return_counts=True)
        del key
        nu = uniq.shape[0]
        least = torch.full((nu,), pts.shape[0], dtype=torch.int64, device=dev)
        least.scatter_reduce_(0, inv, torch.arange(pts.shape[0], dtype=torch.int64, device=dev), "amin")
        order = torch.argsort(least)
        rank = torch.empty_like(order)
        rank[order] = torch.arange(nu, dtype=torch.int64, device=dev)
        eu, ev = [], []
        for off in forward_offsets(conn):
            other = uniq + off
            at = torch.searchsorted(uniq, other).clamp_(max=nu - 1)
            hit = torch.nonzero(uniq[at] == other).reshape(-1)
            eu.append(rank[hit]); ev.append(rank[at[hit]])
        u, w = torch.cat(eu), torch.cat(ev)
        del eu, ev
        par = torch.arange(nu, dtype=torch.int64, device=dev)
        while u.shape[0]:
            pu, pw = par[u], par[w]
            open_ = pu != pw
            u, w, pu, pw = u[open_], w[open_], pu[open_], pw[open_]
            if u.shape[0] == 0:
                break
            m = torch.minimum(pu, pw)
            par.scatter_reduce_(0, pu, m, "amin")
            par.scatter_reduce_(0, pw, m, "amin")
            while True:
                q = par[par]
                if torch.equal(q, par):
                    break
                par = q
        root = par[rank]                            # per voxel (uniq's order): the rank of its component's first voxel
        size = torch.zeros(nu, dtype=torch.int64, device=dev).index_add_(0, root, own)
        return pts, least[order][root][inv], size[root][inv]

    PIECE = 1 << 24                 # rows per gather and per comparison: one indexing call over 1e8 rows (1.6 GB out) came back wrong in places

    def torch_components(ctx, cell, conn, min_points, mode):
        pts, label, size = torch_label(ctx, cell, conn)
        rows = torch.nonzero((size < min_points) == (mode == N.COMPONENTS_SMALL)).reshape(-1)
        out = torch.empty((rows.shape[0], 4), dtype=torch.int32, device=dev)
        for i in range(0, rows.shape[0], PIECE):
            out[i:i + PIECE] = pts[rows[i:i + PIECE]]
        labels = label[rows]
        torch.cuda.synchronize()
        return out, rows, labels

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

        row = {"cells": {}}
        ctx.batch_point_bounds()                            # (the exact boxes: once per context, tools/bench_select.py times it)
        for cell in cells:
            vox = P.as_voxels((0, 0, 0, cell))
            cnt, dst, cst = C.c_int64(), N.DenoiseStats(), N.ComponentsStats()

            def denoise(points=None, rows=None, cap=0):
                chk(ctx, ctx.lib.pcr_denoise(ctx.h, 0, -1, C.byref(vox), None, NEVER, N.DENOISE_KEEP, C.c_void_p(points), C.c_void_p(rows), cap, C.byref(cnt),
                                             C.byref(dst)), "pcr_denoise")

            # the yardstick first: pcr_denoise KEEP at the same cell, all 26 lookups per voxel (it keeps nothing: count = points = rows)
            denoise()
            if cnt.value != 0:
                sys.exit(f"{name} cell {cell}: pcr_denoise with an unreachable max_count keeps {cnt.value} records")
            scratch = torch.empty((16, 4), dtype=torch.int32, device=dev)
            scratch_rows = torch.empty(16, dtype=torch.int64, device=dev)
            dr = {"voxels": dst.as_dict()["voxels"]}
            for label, a in (("count", (None, None, 0)), ("points", (scratch.data_ptr(), None, 16)), ("labels", (scratch.data_ptr(), scratch_rows.data_ptr(), 16))):
                dr[label + "_ms"] = round(timed(lambda: denoise(*a)), 4)
            crow = {"denoise_all_lookups": dr}
            for conn in (6, 26):
                _, _, size = torch_label(ctx, cell, conn)
                min_points = int(torch.sort(size).values[size.shape[0] // 2])
                del size

                def call(mode, points=None, rows=None, labels=None, cap=0):
                    chk(ctx, ctx.lib.pcr_components(ctx.h, 0, -1, C.byref(vox), None, conn, min_points, mode, C.c_void_p(points), C.c_void_p(rows),
                                                    C.c_void_p(labels), cap, C.byref(cnt), C.byref(cst)), "pcr_components")

                for mode in (N.COMPONENTS_SMALL, N.COMPONENTS_KEEP):        # every timed form is checked first, and the other mode once
                    want, want_rows, want_labels = torch_components(ctx, cell, conn, min_points, mode)
                    k = want.shape[0]
                    out = torch.empty((k, 4), dtype=torch.int32, device=dev)
                    out_rows = torch.empty(k, dtype=torch.int64, device=dev)
                    out_labels = torch.empty(k, dtype=torch.int64, device=dev)
                    torch.cuda.synchronize()
                    forms = (("count", (None, None, None, 0)), ("points", (out.data_ptr(), None, None, k)),
                             ("labels", (out.data_ptr(), out_rows.data_ptr(), out_labels.data_ptr(), k)))
                    for _, a in forms:
                        call(mode, *a)
                        if cnt.value != k or (a[0] and not same(out, want)) or (a[1] and not same(out_rows, want_rows)) or (a[2] and not same(out_labels, want_labels)):
                            sys.exit(f"{name} cell {cell} connectivity {conn} mode {mode}: pcr_components differs from the torch alternative")
                    del want, want_rows, want_labels
                    if mode == N.COMPONENTS_SMALL:
                        del out, out_rows, out_labels
                stats = cst.as_dict()
                r = {"min_points": min_points, "written": k, **{s: stats[s] for s in ("voxels", "components", "components_small", "points_small", "largest_points",
                                                                                   "runs", "table_slots")}}
                for label, a in forms:
                    t = timed(lambda: call(N.COMPONENTS_KEEP, *a))
                    r[label + "_ms"] = round(t, 4)
                    r[label + "_ratio_to_denoise"] = round(t / dr[label + "_ms"], 3)
                r["link_ms"] = round(r["count_ms"] - dr["count_ms"], 4)
                r["write_ms"] = round(r["points_ms"] - r["count_ms"], 4)
                r["rows_and_labels_ms"] = round(r["labels_ms"] - r["points_ms"], 4)
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    call(N.COMPONENTS_KEEP, *forms[2][1])
                host_ms = (time.perf_counter() - t0) * 1e3 / args.steps
                t0 = time.perf_counter()
                for _ in range(args.torch_reps):
                    torch_components(ctx, cell, conn, min_points, N.COMPONENTS_KEEP)
                t_alt = (time.perf_counter() - t0) * 1e3 / args.torch_reps
                r.update(labels_host_ms=round(host_ms, 4), decode_plus_torch_host_ms=round(t_alt, 4), speedup_over_torch=round(t_alt / host_ms, 2))
                crow[f"conn{conn}"] = r
                print(f"{name} cell {cell} connectivity {conn}: {r}", file=sys.stderr, flush=True)
                del out, out_rows, out_labels
                torch.cuda.empty_cache()
            row["cells"][str(cell)] = crow
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
