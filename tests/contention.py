"""Streams, frames and trace-derived figures shared by tests/test_contention_cpu.py and tests/test_gpu_contention.py: the
constructed scenes of tests/scenes.py encoded once per process, the three frames rebuilt in numpy from the oracle's point
trace, and the counts the tests state their preconditions with (depth ties, the 1 % edge). CPU only; no expectations here."""
from __future__ import annotations

import functools

import numpy as np

import pcrhpg24_amd as P
from pcrhpg24_amd._native import fb_elems
from tests import las_hqs_ref, oracle, scenes

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
U32 = np.uint64(0xFFFFFFFF)
EDGE_RADIUS = 10000.0
CORNER_TARGET = (177.0, 510.3, 1.0)         # one_pixel_camera(target=...): the cloud lies across the corner of pixels 1136 1137 1201 1202


# ---- streams ---------------------------------------------------------------------------------------------------------
def _points(name: str):
    if name.startswith("tie_planes"):
        return scenes.tie_planes()
    if name.startswith("tie_clusters"):
        return scenes.tie_clusters()
    if name.startswith("edge"):
        return scenes.hqs_edge()[:5]
    if name.startswith("one"):
        return scenes.one_pixel(3)
    if name.startswith("twenty"):
        return scenes.one_pixel(20)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def stream(name: str):
    """(image, OracleFile) of a scene. Name = scene [+ "_unsorted"] [+ "_bc7"]; the edge and one-pixel scenes are written with
    padded chain tails (exactly the points given, no garbage tails), the clusters in the order scenes.tie_clusters gives them."""
    x, y, z, c, las = _points(name)
    pad = name.startswith(("edge", "one", "twenty"))
    image, _ = P.encode_points(x, y, z, c, las, morton_sort="_unsorted" not in name and not name.startswith("tie_clusters"), nthreads=4, pad_tails=pad, bc7=name.endswith("_bc7"))
    return image, oracle.OracleFile(image.view())


@functools.lru_cache(maxsize=None)
def las_cloud(name: str):
    """The 10-10-10 form (P.las_quantize) of a scene, points in input order. The method skips its last batch, so the one-pixel
    cloud gets a fourth."""
    if name == "edge":
        pts = scenes.hqs_edge(outliers=True)[:5]
    elif name == "one":
        pts = scenes.one_pixel(4)
    else:
        pts = _points(name)
    return P.las_quantize(*pts)


FRAMES = {
    "tie_320": lambda: scenes.tie_planes_camera(320, 200),                 # every batch on the double path
    "tie_64": lambda: scenes.tie_planes_camera(64, 36),                    # float path, up to 72 points per pixel
    "clusters_1080": lambda: scenes.tie_clusters_camera(1920, 1080),
    "clusters_4096": lambda: scenes.tie_clusters_camera(4096, 4096),
    "edge_320": lambda: scenes.straight_down(EDGE_RADIUS, scenes.hqs_edge()[5], 320, 200, far=1.0e6),
    "edge_64": lambda: scenes.straight_down(EDGE_RADIUS, scenes.hqs_edge()[5], 64, 36, far=1.0e6),
    "edge_double": lambda: scenes.straight_down(EDGE_RADIUS, scenes.hqs_edge()[5], 320, 200, far=1.0e6, fovy=15.0),   # batches 107 px wide
    "edge_las": lambda: scenes.straight_down(EDGE_RADIUS, scenes.hqs_edge(outliers=True)[5], 320, 200, far=1.0e6),
    "one": lambda: scenes.one_pixel_camera(),
    "corner": lambda: scenes.one_pixel_camera(target=CORNER_TARGET),
}


def frame(name: str) -> P.RenderParams:
    return FRAMES[name]()


# ---- the trace, and the frames rebuilt from it -----------------------------------------------------------------------
def trace(of: oracle.OracleFile, p, variant: int):
    """(pix, depth bits, colour, batch) of every inside point: pcr_oracle_trace_points batch by batch."""
    parts = [of.trace_points(p, variant, first=b, count=1) for b in range(of.num_batches)]
    batch = np.concatenate([np.full(len(t[0]), b, np.int64) for b, t in enumerate(parts)])
    return tuple(np.concatenate([t[k] for t in parts]) for k in range(3)) + (batch,)


def rebuild_basic(of, p) -> np.ndarray:
    """Per-pixel min of depth << 32 | colour over the trace (np.minimum.at)."""
    pix, depth, colour, _ = trace(of, p, oracle.MEM_ITER)
    fb = np.full(fb_elems(p.width, p.height), EMPTY, np.uint64)
    np.minimum.at(fb, pix, (depth.astype(np.uint64) << np.uint64(32)) | colour.astype(np.uint64))
    return fb


def rebuild_hqs(of, p, payload=None):
    """(depth frame, RG, BA) of the two HQS passes from the trace: per-pixel min depth (payload 0, or `payload` per batch), then
    np.add.at over the points with float64(w) <= float64(d) * 1.01."""
    pix, depth, colour, batch = trace(of, p, oracle.HQS)
    n = fb_elems(p.width, p.height)
    fb = np.full(n, EMPTY, np.uint64)
    pay = np.zeros(len(pix), np.uint64) if payload is None else np.asarray(payload, np.uint64)[batch]
    np.minimum.at(fb, pix, (depth.astype(np.uint64) << np.uint64(32)) | pay)
    d = (fb >> np.uint64(32)).astype(np.uint32).view(np.float32)
    with np.errstate(invalid="ignore"):
        passing = depth.view(np.float32).astype(np.float64) <= d[pix].astype(np.float64) * 1.01
    r, g, b = (((colour >> np.uint32(s)) & np.uint32(255)).astype(np.uint64) for s in (0, 8, 16))
    rg, ba = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    np.add.at(rg, pix[passing], ((r << np.uint64(32)) | g)[passing])
    np.add.at(ba, pix[passing], ((b << np.uint64(32)) | np.uint64(1))[passing])
    return fb, rg, ba


def tie_stats(pix, depth, tag, batch, n: int) -> dict:
    """Of the pixels drawn: how many have a winning depth shared by points of different `tag` (colour, or point index), and how
    many by points of different batches."""
    dmin = np.full(n, 0xFFFFFFFF, np.uint32)
    np.minimum.at(dmin, pix, depth)
    tied = depth == dmin[pix]

    def spread(v):
        lo, hi = np.full(n, np.iinfo(np.int64).max, np.int64), np.full(n, -1, np.int64)
        np.minimum.at(lo, pix[tied], v[tied].astype(np.int64))
        np.maximum.at(hi, pix[tied], v[tied].astype(np.int64))
        return int((hi > lo).sum())
    return {"drawn": int(np.unique(pix).size), "other_tag": spread(tag), "other_batch": spread(batch),
            "max_per_pixel": int(np.bincount(pix).max())}


@functools.lru_cache(maxsize=None)
def huffman_tie_stats(stream_name: str, frame_name: str, variant: int = oracle.MEM_ITER) -> dict:
    of, p = stream(stream_name)[1], frame(frame_name)
    pix, depth, colour, batch = trace(of, p, variant)
    return tie_stats(pix, depth, colour, batch, fb_elems(p.width, p.height))


@functools.lru_cache(maxsize=None)
def las_tie_stats(cloud_name: str, frame_name: str) -> dict:
    q, p = las_cloud(cloud_name), frame(frame_name)
    pix, w, index = las_hqs_ref.drawn_points(*q[:4], p, with_index=True)
    return tie_stats(pix, w.view(np.uint32), index, index >> np.uint32(16), fb_elems(p.width, p.height))


def edge_stats(pix, w, n: int, radius: float = EDGE_RADIUS) -> dict:
    """The 1 % test of every drawn point against its pixel's depth d (the nearest point): how many points the f64 form
    float64(w) <= float64(d) * 1.01 and the f32 product w <= float32(d * float32(1.01)) decide differently, and which share
    of the lower layer (w more than 0.5 % behind the top layer's plane) passes the f64 form."""
    d = np.full(n, np.inf, np.float32)
    np.minimum.at(d, pix, w)
    dd = d[pix]
    f64 = w.astype(np.float64) <= dd.astype(np.float64) * 1.01
    f32 = w <= (dd * np.float32(1.01)).astype(np.float32)
    lower = w > np.float32(radius * 1.005)
    return {"differ": int((f64 != f32).sum()), "differ_pixels": int(np.unique(pix[f64 != f32]).size), "lower": int(lower.sum()),
            "lower_passing": float(f64[lower].mean()) if lower.any() else 0.0, "pixels": int(np.unique(pix).size)}


@functools.lru_cache(maxsize=None)
def huffman_edge_stats(stream_name: str, frame_name: str) -> dict:
    of, p = stream(stream_name)[1], frame(frame_name)
    pix, depth, _, _ = trace(of, p, oracle.HQS)
    return edge_stats(pix, depth.view(np.float32), fb_elems(p.width, p.height))


@functools.lru_cache(maxsize=None)
def las_edge_stats(cloud_name: str, frame_name: str) -> dict:
    q, p = las_cloud(cloud_name), frame(frame_name)
    pix, w = las_hqs_ref.drawn_points(*q[:4], p)
    return edge_stats(pix, w, fb_elems(p.width, p.height))


def white_sums(count) -> tuple:
    """(RG, BA) words of `count` pure white points that all pass the 1 % test: 255 * count three times, and the count."""
    count = np.asarray(count, np.uint64)
    s = np.uint64(255) * count
    return (s << np.uint64(32)) | s, (s << np.uint64(32)) | count
