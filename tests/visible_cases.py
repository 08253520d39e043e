"""Cases and the numpy reference of the visible-selection tests (tests/test_visible_cpu.py: the preconditions, from the oracle
alone; tests/test_gpu_visible.py: pcr_select_visible / pcr_read_visible against this reference). Inputs and reference arithmetic
only.

The reference works on the (points, hits) of a screen selection of the WHOLE image -- Context.read_screen(p, None) on the GPU,
oracle_hits() on the CPU -- and restates the definitions of include/pcr_hip.h in numpy: the front depth D by np.minimum.at, the
dilated depth Dr by a padded sliding minimum over the square window, the surface test as float64(w) <= float64(dr) * 1.01, FRONT
as a lexsort by (pixel, depth, colour, index) and the first of each pixel."""
from __future__ import annotations

import functools
import math

import numpy as np

import pcrhpg24_amd as P
from tests import contention, oracle, scenes
from tests import screen_cases as SC

NONE = np.uint32(0xFFFFFFFF)
MODES = {"front": P.VISIBLE_FRONT, "surface": P.VISIBLE_SURFACE}
RADII = (0, 1, 2, 8)

EXTRA_ROW_RADIUS, EXTRA_ROW_HALF = 10000.0, 600.0


def extra_row_scene(seed: int = 21, n: int = 4 * 65536, extent: int = 2_000_000):
    """A thin layer seen straight down from EXTRA_ROW_RADIUS by a camera whose frustum is 2 x EXTRA_ROW_HALF metres high, half of
    its points within 6 cm of the frustum's upper edge: a few dozen of them project to ndc y == 1.0 exactly, pass the inside test
    and land in row `height`, the framebuffer's extra row. Returns the points and the camera's target."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, extent, n).astype(np.int32)
    y = rng.integers(extent // 2 - 700_000, extent // 2 + 700_000, n).astype(np.int32)
    near = rng.integers(0, 2, n) == 0
    y[near] = extent // 2 + int(EXTRA_ROW_HALF / 0.001) + rng.integers(-60, 61, int(near.sum()))
    z = (50_000 + rng.integers(-32, 33, n)).astype(np.int32)
    c = rng.integers(0, 1 << 24, n).astype(np.uint32)
    las = scenes.lattice_las((0, 0, int(z.min())), (extent, extent, int(z.max())), 0.001)
    return x, y, z, c, las, (extent / 2 * 0.001, extent / 2 * 0.001, (50_000 - int(z.min())) * 0.001)


def extra_row_camera(width: int = 64, height: int = 36):
    fovy = 2.0 * math.degrees(math.atan(EXTRA_ROW_HALF / EXTRA_ROW_RADIUS))
    return scenes.straight_down(EXTRA_ROW_RADIUS, extra_row_scene()[5], width, height, far=1.0e6, fovy=fovy)


@functools.lru_cache(maxsize=None)
def _extra_row_stream():
    x, y, z, c, las, _ = extra_row_scene()
    return P.encode_points(x, y, z, c, las, morton_sort=True, nthreads=4, pad_tails=True, bc7=False)[0]


def stream(name: str):
    """The .huffman image of a named stream: "extra_row", or one of tests/screen_cases.py's."""
    return _extra_row_stream().view() if name == "extra_row" else SC.stream(name)


@functools.lru_cache(maxsize=None)
def oracle_file(name: str) -> oracle.OracleFile:
    return oracle.OracleFile(stream(name))


# name -> (stream, camera). The first block are the cameras of tests/screen_cases.py; the frames of tests/contention.py follow.
CASES = {
    "tie_all": ("tie_planes", lambda: SC.CASES["tie_all"][1]()),                # 64 x 36, 256 hits a pixel on four depths
    "tie_all_bc7": ("tie_planes_bc7", lambda: SC.CASES["tie_all_bc7"][1]()),
    "synth_far_lod": ("synth", lambda: SC.CASES["synth_far_lod"][1]()),         # npr = 6
    "synth_cull": ("synth", lambda: SC.CASES["synth_cull"][1]()),               # a batch culled, the f64 path
    "synth_inside": ("synth", lambda: SC.CASES["synth_inside"][1]()),           # points with w <= 0 in kept batches
    "garbage_tail": ("garbage_tail", lambda: SC.CASES["garbage_tail"][1]()),    # the tail artefact: hits anywhere on the screen
    "tie_64": ("tie_planes", lambda: contention.frame("tie_64")),               # a perspective view of the planes: dilation matters
    "edge_64": ("edge", lambda: contention.frame("edge_64")),                   # two layers 1 % apart: the f64 and f32 rules differ
    "edge_double": ("edge", lambda: contention.frame("edge_double")),           # ... on the f64 dequantisation path, 320 x 200
    "extra_row": ("extra_row", extra_row_camera),                               # hits with pixel >= width * height
}
# the frames on which SURFACE at radius 0 is cross-checked against the HQS accumulators (both LOD expressions agree there:
# tests/test_visible_cpu.py)
ACCUM_CASES = ["tie_all", "tie_all_bc7", "tie_64", "edge_64", "edge_double"]


def case(name: str):
    """(stream name, OracleFile, params)."""
    sname, cam = CASES[name]
    return sname, oracle_file(sname), cam()


def rects(p) -> dict:
    """The rects every case runs with: the whole image, an inner rect, one whose window grown by a radius of 2 or more crosses the
    image border on all four sides, and one that lies partly outside the image."""
    w, h = p.width, p.height
    return {"whole": None, "inner": (w // 4, h // 4, (3 * w) // 4, (3 * h) // 4), "border": (1, 1, w - 2, h - 2), "outside": (-7, -5, w // 2, h // 3)}


def batch_reference(sname: str, p, b: int) -> dict:
    """tests/screen_cases.py's batch_reference for the streams of this module as well."""
    if sname != "extra_row":
        return SC.batch_reference(sname, p, b)
    of = oracle_file(sname)
    drawn, npr, dbl = of.batch_lod(b, p)
    assert drawn and npr == 64, "the extra-row camera draws every point of every batch"
    pix, depth, colour = of.trace_points(p, first=b, count=1)
    full = len(pix) == npr * 1024
    return {"drawn": True, "npr": npr, "double": dbl, "pix": pix, "depth": depth, "colour": colour & np.uint32(0xFFFFFF), "full": full,
            "index": SC.trace_index(b, npr) if full else None}


@functools.lru_cache(maxsize=None)
def oracle_hits(name: str):
    """(points, hits, exact) of the whole image from the oracle's trace, shaped and ordered as Context.read_screen's (of a record
    only the colour is filled in). exact: every drawn batch's trace names its records; otherwise the index of a batch that is
    partly outside the frustum is its trace position, which orders the batch's hits but names no record."""
    sname, of, p = case(name)
    pix, depth, colour, index, exact = [], [], [], [], True
    for b in range(of.num_batches):
        r = batch_reference(sname, p, b)
        pix.append(r["pix"]); depth.append(r["depth"]); colour.append(r["colour"])
        if r["index"] is None:
            exact = exact and len(r["pix"]) == 0
            index.append(b * SC.PPB + np.arange(len(r["pix"]), dtype=np.int64))
        else:
            index.append(r["index"])
    pix, depth, colour, index = (np.concatenate(v) for v in (pix, depth, colour, index))
    order = np.argsort(index, kind="stable")
    pts, hits = np.zeros(len(order), P.POINT_DTYPE), np.zeros(len(order), P.HIT_DTYPE)
    pts["color"] = colour[order]
    hits["pixel"], hits["depth_bits"], hits["index"] = pix[order], depth[order], index[order]
    return pts, hits, exact


def dilate(d: np.ndarray, radius: int) -> np.ndarray:
    """Min of the uint32 plane d [h, w] over the square window of `radius` pixels, clipped to the image (a padded sliding minimum)."""
    h, w = d.shape
    padded = np.pad(d, radius, constant_values=NONE)
    out = d.copy()
    for dy in range(2 * radius + 1):
        for dx in range(2 * radius + 1):
            np.minimum(out, padded[dy:dy + h, dx:dx + w], out=out)
    return out


class Reference:
    """The definitions over one whole-image screen selection. Nothing here is changed after it has been worked out."""

    def __init__(self, pts, hits, p):
        self.pts, self.hits, self.p = pts, hits, p
        self.width, self.height, self.n = p.width, p.height, p.width * p.height
        self.pix = hits["pixel"].astype(np.int64)
        self.depth, self.colour, self.index = hits["depth_bits"], pts["color"], hits["index"]
        self.in_image = self.pix < self.n                   # (the framebuffer's extra row takes part in nothing)
        d = np.full(self.n, NONE, np.uint32)
        np.minimum.at(d, self.pix[self.in_image], self.depth[self.in_image])
        self.front_depth = d.reshape(self.height, self.width)
        self.covered = int((d != NONE).sum())
        self._planes, self._passing, self._first = {}, {}, None

    def plane(self, radius: int) -> np.ndarray:
        """Dr as uint32 [height, width]."""
        if radius not in self._planes:
            self._planes[radius] = dilate(self.front_depth, radius)
            self._planes[radius].setflags(write=False)
        return self._planes[radius]

    def passing(self, radius: int) -> np.ndarray:
        """Mask over the hits: in the image and float64(w) <= float64(dr) * 1.01."""
        if radius not in self._passing:
            w = self.depth.view(np.float32)
            dr = self.plane(radius).reshape(-1)[np.minimum(self.pix, self.n - 1)].view(np.float32)
            with np.errstate(invalid="ignore"):
                self._passing[radius] = self.in_image & (w.astype(np.float64) <= dr.astype(np.float64) * 1.01)
        return self._passing[radius]

    def passing_f32(self, radius: int) -> np.ndarray:
        """The same with the f32 product w <= d * 1.01f: what the rule is NOT."""
        w = self.depth.view(np.float32)
        dr = self.plane(radius).reshape(-1)[np.minimum(self.pix, self.n - 1)].view(np.float32)
        with np.errstate(invalid="ignore"):
            return self.in_image & (w <= (dr * np.float32(1.01)).astype(np.float32))

    def first(self) -> np.ndarray:
        """Mask over the hits: of every pixel of the image the hit that is least by (depth_bits, colour, index)."""
        if self._first is None:
            pos = np.nonzero(self.in_image)[0]
            order = pos[np.lexsort((self.index[pos], self.colour[pos], self.depth[pos], self.pix[pos]))]
            head = np.ones(len(order), bool)
            head[1:] = self.pix[order][1:] != self.pix[order][:-1]
            self._first = np.zeros(len(self.pix), bool)
            self._first[order[head]] = True
        return self._first

    def in_rect(self, rect) -> np.ndarray:
        return self.in_image & SC.in_rect(self.pix, self.p, rect)

    def select(self, rect, mode: str, radius: int):
        """(mask of the selected hits, the stats fields the definitions give)."""
        cand = self.in_rect(rect)
        sel = cand & self.passing(radius)
        if mode == "front":
            sel = sel & self.first()
        st = {"hits": int(self.in_image.sum()), "pixels_covered": self.covered, "candidates": int(cand.sum()), "selected": int(sel.sum())}
        return sel, st


@functools.lru_cache(maxsize=None)
def oracle_reference(name: str) -> Reference:
    pts, hits, _ = oracle_hits(name)
    return Reference(pts, hits, case(name)[2])


def lod_agrees(name: str) -> bool:
    """Do the basic method's and the HQS method's LOD expressions decide every batch of the case alike?"""
    sname, of, p = case(name)
    return all(of.batch_lod(b, p, oracle.MEM_ITER) == of.batch_lod(b, p, oracle.HQS) for b in range(of.num_batches))
