"""Visible selection, the parts that need no GPU: the two entry points and the stats struct in the headers, the binding table and
the cross-compiled library; the CLI's refusal of a malformed --visible before any device is touched; and the preconditions of
tests/test_gpu_visible.py from the oracle alone -- the cases of tests/visible_cases.py make every rule of the definition decide.
Each condition is asserted, not assumed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import _native as N
from pcrhpg24_amd import build
from tests import screen_cases as SC
from tests import visible_cases as V
from tests.test_abi import declared

SYMBOLS = ("pcr_select_visible", "pcr_read_visible")


def test_entry_points_are_declared_bound_and_exported():
    for name in SYMBOLS:
        assert name in declared("pcr_hip.h") and name in N.HIP_SYMBOLS
    build.build_hip()
    lib = C.CDLL(build.HIP_LIB)
    for name in SYMBOLS:
        assert hasattr(lib, name)
    bound = N.hip_lib()
    want = [C.c_void_p, C.POINTER(N.RenderParams), C.POINTER(N.Rect), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
            C.POINTER(C.c_int64), C.POINTER(N.VisibleStats)]
    assert bound.pcr_select_visible.argtypes == want and bound.pcr_read_visible.argtypes == want
    for name in ("VisibleStats", "VISIBLE_FRONT", "VISIBLE_SURFACE", "VISIBLE_MAX_RADIUS"):
        assert hasattr(P, name)
    for name in ("select_visible", "read_visible"):
        assert callable(getattr(P.Context, name))
    assert (P.Context.VISIBLE_FRONT, P.Context.VISIBLE_SURFACE) == (P.VISIBLE_FRONT, P.VISIBLE_SURFACE)
    assert callable(P.HuffmanLasData.visible_points)


def test_struct_and_constants_match_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pcr_types.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %d %d %d\\n", sizeof(pcr_visible_stats),\n'
                   'offsetof(pcr_visible_stats, batches_skipped), offsetof(pcr_visible_stats, batches_decoded), offsetof(pcr_visible_stats, hits),\n'
                   'offsetof(pcr_visible_stats, pixels_covered), offsetof(pcr_visible_stats, candidates), offsetof(pcr_visible_stats, selected),\n'
                   'PCR_VISIBLE_FRONT, PCR_VISIBLE_SURFACE, PCR_VISIBLE_MAX_RADIUS); return 0; }\n')
    subprocess.run(["gcc", "-I", build.INCLUDE, str(src), "-o", str(tmp_path / "layout")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "layout")], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert got[:7] == [48, 0, 8, 16, 24, 32, 40]
    assert [C.sizeof(N.VisibleStats)] + [getattr(N.VisibleStats, f).offset for f, _ in N.VisibleStats._fields_] == got[:7]
    assert got[7:] == [P.VISIBLE_FRONT, P.VISIBLE_SURFACE, P.VISIBLE_MAX_RADIUS] == [0, 1, 8]
    assert max(V.RADII) == P.VISIBLE_MAX_RADIUS and min(V.RADII) == 0


# ---- the CLI -----------------------------------------------------------------------------------------------------------------
NO_DEVICE = dict(os.environ, HIP_VISIBLE_DEVICES="-1")


@pytest.mark.parametrize("args", [["--visible", "front"], ["--view", "--visible"], ["--view", "--visible", "nearest"], ["--view", "--occluder", "2"],
                                  ["--view", "--visible", "front", "--occluder"], ["--view", "--visible", "front", "--occluder", "9"],
                                  ["--view", "--visible", "front", "--occluder", "-1"], ["--view", "--visible", "surface", "--occluder", "1.5"],
                                  ["--view", "--visible", "front", "--visible", "surface"], ["--box", "0", "0", "0", "1", "1", "1", "--visible", "front"]])
def test_decode_cli_refuses_a_malformed_visible_before_it_creates_a_context(tmp_path, args):
    build.build_tools()
    out = tmp_path / "out.las"
    # (the input does not exist and HIP sees no device: either would be the message if the tool got that far)
    res = subprocess.run([build.DECODE_BIN, str(tmp_path / "missing.huffman"), str(out), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=120, env=NO_DEVICE)
    assert res.returncode == 2 and res.stderr.startswith("usage: pcr_decode") and "--visible front|surface [--occluder R]" in res.stderr
    assert "pcr_create" not in res.stderr and "missing.huffman" not in res.stderr and not out.exists()


# ---- the reference itself ------------------------------------------------------------------------------------------------------
def test_dilate_is_the_window_minimum_clipped_to_the_image():
    rng = np.random.default_rng(5)
    d = rng.integers(0, 1 << 32, (7, 11), dtype=np.uint64).astype(np.uint32)
    d[rng.random(d.shape) < 0.4] = V.NONE
    assert np.array_equal(V.dilate(d, 0), d)
    for radius in (1, 2, 8):
        got = V.dilate(d, radius)
        for y in range(d.shape[0]):
            for x in range(d.shape[1]):
                assert got[y, x] == d[max(y - radius, 0):y + radius + 1, max(x - radius, 0):x + radius + 1].min()


# ---- preconditions of the GPU cases --------------------------------------------------------------------------------------------
def per_pixel(R, mask):
    return np.bincount(R.pix[mask], minlength=R.n)


def test_tie_all_makes_the_surface_rule_and_the_index_decide():
    R = V.oracle_reference("tie_all")
    assert V.oracle_hits("tie_all")[2] and len(R.pix) == 262144 and R.covered == 1024
    sel, st = R.select(None, "surface", 0)
    total, passing = per_pixel(R, R.in_image), per_pixel(R, sel)
    covered = total > 0
    assert ((passing[covered] > 1) & (passing[covered] < total[covered])).all(), "SURFACE selects one hit or all hits of some pixel"
    # pixels whose front depth AND colour is shared by several hits: only the index decides FRONT there
    key = SC.key_of(R.depth, R.colour)
    front_key = np.full(R.n, np.uint64(0xFFFFFFFFFFFFFFFF))
    np.minimum.at(front_key, R.pix, key)
    tied = per_pixel(R, key == front_key[R.pix])
    assert int((tied > 1).sum()) == 415
    first, st = R.select(None, "front", 0)
    assert st["selected"] == 1024 and (per_pixel(R, first)[covered] == 1).all()
    px, py = SC.PICK_TIE
    assert tied[px + py * R.width] > 1


def test_bc7_case_has_index_ties_too():
    R = V.oracle_reference("tie_all_bc7")
    key = SC.key_of(R.depth, R.colour)
    front_key = np.full(R.n, np.uint64(0xFFFFFFFFFFFFFFFF))
    np.minimum.at(front_key, R.pix, key)
    assert int((per_pixel(R, key == front_key[R.pix]) > 1).sum()) > 0


@pytest.mark.parametrize("name,differ", [("edge_64", 1037), ("edge_double", 966)])
def test_the_f64_rule_and_the_f32_product_disagree(name, differ):
    R = V.oracle_reference(name)
    assert int((R.passing(0) != R.passing_f32(0)).sum()) == differ
    if name == "edge_double":
        sname, of, p = V.case(name)
        assert all(of.batch_lod(b, p)[2] for b in range(of.num_batches)), "a batch of edge_double is not on the f64 path"


@pytest.mark.parametrize("name,counts,uncovered", [("tie_64", (90857, 79982, 69966), (0, 23, 93)), ("edge_double", (207190, 196872, 196154), None)])
def test_dilation_matters(name, counts, uncovered):
    R = V.oracle_reference(name)
    for radius, want in zip((0, 1, 2), counts):
        sel, st = R.select(None, "surface", radius)
        assert st["selected"] == want
        if uncovered is not None:
            # covered pixels left without any selected hit: FRONT's second clause (the winner must pass the surface test) bites
            assert R.covered - np.unique(R.pix[sel]).size == uncovered[radius]
            assert R.select(None, "front", radius)[1]["selected"] == R.covered - uncovered[radius]


def test_dilation_does_nothing_on_edge_64():
    R = V.oracle_reference("edge_64")
    masks = [R.select(None, "surface", radius)[0] for radius in V.RADII]
    assert int(masks[0].sum()) == 196039
    for m in masks[1:]:
        assert np.array_equal(m, masks[0])


@pytest.mark.parametrize("name", V.ACCUM_CASES)
def test_lod_expressions_agree_on_the_accumulator_frames(name):
    assert V.lod_agrees(name)


def test_border_windows_are_clipped_on_all_four_sides():
    """The border rect's window, grown by the radius, crosses the image border on every side, candidates lie within the radius of
    every side, and the clipped windows there change the result (radius 2 selects other hits than radius 0 among them)."""
    R = V.oracle_reference("tie_64")
    p = R.p
    rect = V.rects(p)["border"]
    for radius in (2, 8):
        assert rect[0] - radius < 0 and rect[1] - radius < 0 and rect[2] + radius > p.width - 1 and rect[3] + radius > p.height - 1
    cand = R.in_rect(rect)
    x, y = R.pix % p.width, R.pix // p.width
    sides = [cand & (x <= 2), cand & (x >= p.width - 3), cand & (y <= 2), cand & (y >= p.height - 3)]
    s0, s2 = R.select(rect, "surface", 0)[0], R.select(rect, "surface", 2)[0]
    for side in sides:
        assert side.any() and (s0 & side).sum() != (s2 & side).sum()
    out = V.rects(p)["outside"]
    assert out[0] < 0 and out[1] < 0 and 0 < R.select(out, "surface", 0)[1]["candidates"] < len(R.pix)


def test_extra_row_case_has_hits_in_the_framebuffers_extra_row():
    """Hits with pixel >= width * height exist and lie in row `height` (inside the framebuffer, past the planes of the image)."""
    R = V.oracle_reference("extra_row")
    p = R.p
    extra = ~R.in_image
    assert 10 < int(extra.sum()) < len(R.pix) and (R.pix[extra] < N.fb_elems(p.width, p.height)).all() and (R.pix[extra] // p.width == p.height).all()
    sel, st = R.select(None, "surface", 1)
    assert st["hits"] == len(R.pix) - int(extra.sum()) == st["candidates"] and not sel[extra].any()


def test_special_cases_are_what_they_are_named_for():
    # fewer than 64 points per chain
    sname, of, p = V.case("synth_far_lod")
    lods = [of.batch_lod(b, p) for b in range(of.num_batches)]
    assert any(drawn and 0 < npr < 64 for drawn, npr, _ in lods)
    # a culled batch, and drawn batches on the f64 path
    sname, of, p = V.case("synth_cull")
    lods = [of.batch_lod(b, p) for b in range(of.num_batches)]
    assert any(not drawn for drawn, _, _ in lods) and any(drawn and dbl for drawn, _, dbl in lods)
    # points with w <= 0 (or otherwise outside) in kept batches: their traces are incomplete
    sname, of, p = V.case("synth_inside")
    refs = [SC.batch_reference(sname, p, b) for b in range(of.num_batches)]
    assert any(r["drawn"] and not r["full"] for r in refs)
    # the tail artefact: hits far from the rest of the picture, which dilation lets occlude
    R = V.oracle_reference("garbage_tail")
    assert R.select(None, "surface", 1)[1]["selected"] < R.select(None, "surface", 0)[1]["selected"] // 10
    # every case: some but not all hits selected in either mode at radius 0, and an inner rect that holds some but not all
    for name in V.CASES:
        R = V.oracle_reference(name)
        for mode in V.MODES:
            assert 0 < R.select(None, mode, 0)[1]["selected"] < len(R.pix), (name, mode)
