"""Cameras, rects, pick windows and the numpy side of the screen-selection tests (tests/test_screen_cpu.py checks on the CPU, from
the oracle alone, that they make every case occur that tests/test_gpu_screen.py needs). Inputs and reference arithmetic only.

The reference of every comparison is the oracle's point trace of one batch, OracleFile.trace_points(p, first=b, count=1): pixel,
f32 bits of w and colour of every point of the batch that passes the inside test, in walk order -- cluster by cluster, then
point, then lane. When every walked point of a batch is inside (the trace holds npr * 1024 entries) the position tells the
record: trace position (c >> 5) * npr * 32 + i * 32 + (c & 31) is point i of chain c. For the other batches the trace does not
say which points it left out, and only the multiset of (pixel, depth bits, colour) can be compared."""
from __future__ import annotations

import functools

import numpy as np

import pcrhpg24_amd as P
from tests import contention, oracle, scenes
from tests import select_cases as S

PPB = 65536


def stream(name: str):
    """The .huffman image of a named stream: those of tests/select_cases.py and tests/decoder_cases.py, and the scenes of
    tests/contention.py."""
    if name in ("synth", "clustered", "garbage_tail", "escape_heavy", "wide30"):
        return S.stream(name)
    if name.startswith("decoder/"):                     # "decoder/<stream>-<padded|plain>[-bc7]": tests/decoder_cases.py
        from tests import decoder_cases
        return decoder_cases.stream_by_id(name[len("decoder/"):])
    return contention.stream(name)[0].view()


@functools.lru_cache(maxsize=None)
def oracle_file(name: str) -> oracle.OracleFile:
    return oracle.OracleFile(stream(name))


def _orbit(yaw, pitch, radius, target, width, height, lod=100, cull=1, **kw):
    return scenes.with_flags(P.camera_orbit(yaw, pitch, radius, target, width, height, **kw), lod_percent=lod, cull=cull)


# name -> (stream, camera, rect or None). Cameras come from the project's own helper (P.camera_orbit through tests/scenes.py).
CASES = {
    # the 1 km synthetic tile, 10 batches
    "synth_overview": ("synth", lambda: scenes.with_flags(scenes.cameras(160, 90)["overview"], lod_percent=100), None),
    "synth_rect": ("synth", lambda: scenes.with_flags(scenes.cameras(160, 90)["overview"], lod_percent=100), (40, 30, 100, 60)),
    "synth_far_lod": ("synth", lambda: scenes.with_flags(scenes.cameras(160, 90)["far"], lod_percent=10), None),             # npr = 6
    "synth_cull": ("synth", lambda: _orbit(-0.15, -1.2, 600.0, (500.0, 750.0, 40.0), 320, 180), None),       # a batch culled, four partly inside, f64
    "synth_cull_rect": ("synth", lambda: _orbit(-0.15, -1.2, 600.0, (500.0, 750.0, 40.0), 320, 180), (100, 60, 200, 120)),
    # five Gaussian clusters, 5 batches
    "clustered_down": ("clustered", lambda: _orbit(0.0, -np.pi / 2, 1200.0, (500.0, 500.0, 20.0), 200, 200), None),
    "clustered_rect": ("clustered", lambda: _orbit(0.0, -np.pi / 2, 1200.0, (500.0, 500.0, 20.0), 200, 200), (20, 20, 120, 120)),
    "clustered_cull_lod": ("clustered", lambda: _orbit(0.0, -1.5, 700.0, (500.0, 900.0, 20.0), 320, 200, lod=10), None),  # culled, npr 6 and 64, f64
    # one camera each (check 4 of the GPU tests)
    "garbage_tail": ("garbage_tail", lambda: scenes.with_flags(scenes.cameras(160, 90)["overview"], lod_percent=100), (60, 35, 100, 55)),
    "escape_heavy": ("escape_heavy", lambda: _orbit(0.4, -0.8, 5000.0, (1148.0, 1148.0, 1100.0), 160, 90), (70, 40, 90, 50)),
    "wide30": ("wide30", lambda: _orbit(0.0, -np.pi / 2, 2.0e6, (536870.0, 1.0, 0.0), 160, 90, cull=0, far=1.0e7), (100, 0, 159, 89)),
    # outside the preconditioned set: points behind the camera (w <= 0) in batches the cull keeps, none of them wholly inside
    "synth_inside": ("synth", lambda: scenes.with_flags(scenes.cameras(160, 90)["inside"], lod_percent=100), (0, 0, 159, 44)),
    # the tie planes of tests/contention.py seen whole from 200 m: dozens of points per pixel on four depths; and as BC7
    "tie_all": ("tie_planes", lambda: scenes.straight_down(200.0, (100.0, 100.0, 50.0), 64, 36), None),
    "tie_all_bc7": ("tie_planes_bc7", lambda: scenes.straight_down(200.0, (100.0, 100.0, 50.0), 64, 36), (25, 8, 40, 25)),
    "tie_320": ("tie_planes", lambda: contention.frame("tie_320"), (100, 50, 219, 149)),
}
PRECONDITIONED = [k for k, v in CASES.items() if v[0] in ("synth", "clustered") and k != "synth_inside"]
STREAM_CASES = ["garbage_tail", "escape_heavy", "wide30"]


def case(name: str):
    """(stream name, OracleFile, params, rect)."""
    sname, cam, rect = CASES[name]
    return sname, oracle_file(sname), cam(), rect


def clip(p, rect):
    """The rect clipped to the image as (x0, y0, x1, y1), None for the whole image -> the full-image rect; an empty result has
    x0 > x1 or y0 > y1."""
    if rect is None:
        return 0, 0, p.width - 1, p.height - 1
    x0, y0, x1, y1 = (int(v) for v in rect)
    return max(x0, 0), max(y0, 0), min(x1, p.width - 1), min(y1, p.height - 1)


def in_rect(pix, p, rect):
    """Mask of the pixel indices whose column pix % width and row pix // width lie in the rect clipped to the image."""
    x0, y0, x1, y1 = clip(p, rect)
    pix = np.asarray(pix, np.int64)
    x, y = pix % p.width, pix // p.width
    return (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1)


def trace_index(b: int, npr: int):
    """Record index (pcr_decode_points order, batch 0 of the stream first) of every position of a complete trace of batch b."""
    t = np.arange(npr * 1024, dtype=np.int64)
    cl, r = t // (npr * 32), t % (npr * 32)
    return b * PPB + (cl * 32 + r % 32) * 64 + r // 32


@functools.lru_cache(maxsize=64)
def _batch_reference(sname: str, pkey: bytes, b: int):
    of = oracle_file(sname)
    p = P.RenderParams.from_buffer_copy(pkey)
    drawn, npr, dbl = of.batch_lod(b, p)
    drawn = drawn and npr > 0
    if not drawn:
        e = np.zeros(0, np.int64)
        return {"drawn": False, "npr": npr, "double": dbl, "pix": e, "depth": e.astype(np.uint32), "colour": e.astype(np.uint32), "full": False, "index": None}
    pix, depth, colour = of.trace_points(p, first=b, count=1)
    colour = colour & np.uint32(0xFFFFFF)       # a record holds 0x00BBGGRR; the oracle's BC7 decode also returns the block's alpha
    full = len(pix) == npr * 1024
    return {"drawn": True, "npr": npr, "double": dbl, "pix": pix, "depth": depth, "colour": colour, "full": full,
            "index": trace_index(b, npr) if full else None}


def batch_reference(sname: str, p, b: int) -> dict:
    """The oracle's view of batch b under camera p: drawn, npr, double, the trace (pix, depth, colour), full = every walked
    point is inside, and then index = the record of every trace position."""
    return _batch_reference(sname, bytes(p), b)


def reference(sname: str, p, rect):
    """Per batch of the stream the trace restricted to the rect: list of dicts as batch_reference's with the arrays masked
    (index too, where the batch is full) and "partly" = some but not all of the batch's hits are in the rect."""
    of = oracle_file(sname)
    out = []
    for b in range(of.num_batches):
        r = dict(batch_reference(sname, p, b))
        m = in_rect(r["pix"], p, rect)
        r["partly"] = bool(m.any() and not m.all())
        for k in ("pix", "depth", "colour"):
            r[k] = r[k][m]
        if r["index"] is not None:
            r["index"] = r["index"][m]
        out.append(r)
    return out


def key_of(depth, colour):
    return (np.asarray(depth, np.uint64) << np.uint64(32)) | np.asarray(colour, np.uint64)


def sorted_triples(pix, depth, colour):
    """The multiset of (pixel, depth bits, colour) as a sorted [n, 3] array."""
    a = np.stack([np.asarray(pix, np.int64), np.asarray(depth, np.int64), np.asarray(colour, np.int64)], axis=1)
    return a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]


# ---- pick windows --------------------------------------------------------------------------------------------------------------
# A pixel of the tie frame at which, by the oracle, several points share the winning depth bits AND colour (BC1 gives the sixteen
# neighbours of a chain four colours): only the index decides between them. tests/test_screen_cpu.py checks it.
PICK_CASE = "tie_all"
PICK_TIE = (17, 2)
PICK_RADII = (1, 3, 8)


def pick_reference(pix, depth, colour, index, p, px, py, radius):
    """numpy minimum of (depth bits, colour, index) over the hits in the window: (position of the winner, how many hits hold its
    depth bits and colour), or None for an empty window."""
    m = in_rect(pix, p, (px - radius, py - radius, px + radius, py + radius))
    if not m.any():
        return None
    pos = np.nonzero(m)[0]
    order = np.lexsort((index[pos], colour[pos], depth[pos]))
    w = pos[order[0]]
    same = (depth[pos] == depth[w]) & (colour[pos] == colour[w])
    return int(w), int(same.sum())
