"""Screen selection and picking, the parts that need no GPU: the three entry points and three structs in the headers, the binding
tables and the cross-compiled library; the CLI's refusal of malformed --view / --rect / --pick arguments before any device is
touched; and the preconditions of tests/test_gpu_screen.py, from the oracle alone: the cameras of tests/screen_cases.py make
every kind of batch occur, the exact-index check covers at least half of every preconditioned selection, and the tie window
holds points of different index that share depth bits and colour."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import _native as N
from pcrhpg24_amd import build
from tests import screen_cases as SC
from tests.test_abi import declared

SYMBOLS = ("pcr_select_screen", "pcr_read_screen", "pcr_pick")


def test_entry_points_are_declared_bound_and_exported():
    for name in SYMBOLS:
        assert name in declared("pcr_hip.h") and name in N.HIP_SYMBOLS
    build.build_hip()
    lib = C.CDLL(build.HIP_LIB)
    for name in SYMBOLS:
        assert hasattr(lib, name)
    bound = N.hip_lib()
    sel = [C.c_void_p, C.POINTER(N.RenderParams), C.POINTER(N.Rect), C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int64), C.POINTER(N.ScreenStats)]
    assert bound.pcr_select_screen.argtypes == sel and bound.pcr_read_screen.argtypes == sel
    assert bound.pcr_pick.argtypes == [C.c_void_p, C.POINTER(N.RenderParams), C.c_int, C.c_int, C.c_int, C.POINTER(N.Point), C.POINTER(N.ScreenHit),
                                       C.POINTER(C.c_int)]
    for name in ("Rect", "ScreenHit", "ScreenStats", "HIT_DTYPE", "as_rect"):
        assert hasattr(P, name)
    for name in ("select_screen", "read_screen", "pick"):
        assert callable(getattr(P.Context, name))
    assert callable(P.HuffmanLasData.points_on_screen)


def test_structs_match_the_header(tmp_path):
    """sizeof / offsetof as a C compiler sees include/pcr_types.h, against the ctypes mirrors and the numpy dtype."""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pcr_types.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(pcr_rect), offsetof(pcr_rect, x0),\n'
                   'offsetof(pcr_rect, y0), offsetof(pcr_rect, x1), offsetof(pcr_rect, y1), sizeof(pcr_screen_hit), offsetof(pcr_screen_hit, pixel),\n'
                   'offsetof(pcr_screen_hit, depth_bits), offsetof(pcr_screen_hit, index), sizeof(pcr_screen_stats),\n'
                   'offsetof(pcr_screen_stats, batches_skipped), offsetof(pcr_screen_stats, batches_decoded),\n'
                   'offsetof(pcr_screen_stats, points_tested), offsetof(pcr_screen_stats, points_selected)); return 0; }\n')
    subprocess.run(["gcc", "-I", build.INCLUDE, str(src), "-o", str(tmp_path / "layout")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "layout")], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert got == [16, 0, 4, 8, 12, 16, 0, 4, 8, 32, 0, 8, 16, 24]
    assert [C.sizeof(N.Rect)] + [getattr(N.Rect, f).offset for f, _ in N.Rect._fields_] == got[:5]
    assert [C.sizeof(N.ScreenHit)] + [getattr(N.ScreenHit, f).offset for f, _ in N.ScreenHit._fields_] == got[5:9]
    assert [C.sizeof(N.ScreenStats)] + [getattr(N.ScreenStats, f).offset for f, _ in N.ScreenStats._fields_] == got[9:]
    assert P.HIT_DTYPE.itemsize == 16 and [P.HIT_DTYPE.fields[f][1] for f in ("pixel", "depth_bits", "index")] == got[6:9]
    assert C.sizeof(N.SelectStats) == 32 and [f for f, _ in N.SelectStats._fields_] == ["batches_outside", "batches_inside", "batches_straddling", "points_selected"]


def test_as_rect():
    r = P.as_rect((1, 2, 3, 4))
    assert (r.x0, r.y0, r.x1, r.y1) == (1, 2, 3, 4) and P.as_rect(None) is None and P.as_rect(r) is r
    with pytest.raises(ValueError):
        P.as_rect((0, 0, 1 << 31, 0))
    with pytest.raises(ValueError):
        P.as_rect((0, 0, 1))


# ---- the CLI -----------------------------------------------------------------------------------------------------------------
NO_DEVICE = dict(os.environ, HIP_VISIBLE_DEVICES="-1")


@pytest.mark.parametrize("args", [["--view", "--rect"], ["--view", "--rect", "0", "0", "10"], ["--view", "--rect", "0", "0", "10", "x"],
                                  ["--view", "--rect", "0", "0", "10", "1.5"], ["--view", "--rect", "10", "0", "5", "20"],
                                  ["--view", "--rect", "0", "0", "10", "99999999999"], ["--view", "--rect", "0", "0", "1", "1", "--rect", "0", "0", "1", "1"],
                                  ["--rect", "0", "0", "10", "10"], ["--view", "--size", "320"], ["--view", "--size", "0x10"],
                                  ["--view", "--camera", "0", "0", "10", "0", "0"], ["--view", "--camera", "0", "0", "10", "0", "0", "nan"],
                                  ["--view", "--lod", "ten"], ["--view", "--cull", "2"], ["--view", "--vew"],
                                  ["--box", "0", "0", "0", "1", "1", "1", "--view"]])
def test_decode_cli_refuses_a_malformed_view_before_it_creates_a_context(tmp_path, args):
    build.build_tools()
    out = tmp_path / "out.las"
    # (the input does not exist and HIP sees no device: either would be the message if the tool got that far)
    res = subprocess.run([build.DECODE_BIN, str(tmp_path / "missing.huffman"), str(out), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=120, env=NO_DEVICE)
    assert res.returncode == 2 and res.stderr.startswith("usage: pcr_decode") and "--rect x0 y0 x1 y1" in res.stderr
    assert "pcr_create" not in res.stderr and "missing.huffman" not in res.stderr and not out.exists()


@pytest.mark.parametrize("args", [["--pick"], ["--pick", "3"], ["--pick", "3", "x"], ["--pick", "1.5", "2"], ["--pick", "3", "4", "-1"],
                                  ["--pick", "3", "4", "r"], ["--pick", "3", "99999999999"], ["--pick", "3", "4", "5", "6"],
                                  ["--method", "loop_las_cuda", "--pick", "3", "4"]])
def test_render_cli_refuses_a_malformed_pick_before_it_creates_a_context(tmp_path, args):
    build.build_tools()
    res = subprocess.run([build.RENDER_BIN, str(tmp_path / "missing.huffman"), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=120, env=NO_DEVICE)
    assert res.returncode == 2 and res.stderr.strip() and res.stdout == ""
    assert "pcr_create" not in res.stderr and "missing.huffman" not in res.stderr


# ---- preconditions of the GPU cases ------------------------------------------------------------------------------------------
def summary(name):
    sname, of, p, rect = SC.case(name)
    ref = SC.reference(sname, p, rect)
    total = sum(len(r["pix"]) for r in ref)
    exact = sum(len(r["pix"]) for r in ref if r["full"])
    return p, ref, total, exact


@pytest.mark.parametrize("stream", ["synth", "clustered"])
def test_preconditioned_cameras_make_every_kind_of_batch_occur(stream):
    names = [n for n in SC.PRECONDITIONED if SC.CASES[n][0] == stream]
    culled = full = partial = lod_cut = double = partly = False
    for name in names:
        p, ref, total, exact = summary(name)
        culled = culled or any(not r["drawn"] for r in ref)
        full = full or any(r["full"] and len(r["pix"]) for r in ref)
        partial = partial or any(r["drawn"] and not r["full"] and len(r["pix"]) for r in ref)
        lod_cut = lod_cut or (p.lod_percent < 100 and any(r["drawn"] and 0 < r["npr"] < 64 for r in ref))
        double = double or any(r["drawn"] and r["double"] for r in ref)
        partly = partly or any(r["partly"] for r in ref)
    assert culled, "no camera culls a batch"
    assert full, "no batch with every walked point inside: the exact-index check would never apply"
    assert partial, "no batch partly inside the frustum"
    assert lod_cut, "no camera below LOD 100 with a drawn batch of fewer than 64 points per chain"
    assert double, "no drawn batch on the f64 path"
    assert partly, "no rect holds some but not all hits of a batch"


@pytest.mark.parametrize("name", SC.PRECONDITIONED)
def test_hold_out_condition(name):
    """The batches only the multiset check applies to hold at most half of the selected points."""
    p, ref, total, exact = summary(name)
    assert total > 0 and 2 * (total - exact) <= total, (name, total, exact)


@pytest.mark.parametrize("name", SC.STREAM_CASES + ["tie_all", "tie_all_bc7"])
def test_stream_cases_select_some_but_not_all(name):
    sname, of, p, rect = SC.case(name)
    ref = SC.reference(sname, p, rect)
    assert all(r["full"] for r in ref), "every batch of these cases is checked record by record"
    if rect is not None:
        assert any(r["partly"] for r in ref)
        assert 0 < sum(len(r["pix"]) for r in ref) < sum(len(r["pix"]) for r in SC.reference(sname, p, None))


def test_trace_position_names_the_record():
    """The mapping the exact check rests on, against the oracle's decoder: the record the trace position names, dequantised and
    projected in numpy float32 / float64 the way the oracle states it, lands on the traced pixel with the traced depth bits.
    (A level of detail below 64 and a batch on the f64 path included.)"""
    checked = 0
    for name in ("synth_far_lod", "clustered_down"):
        sname, of, p, _ = SC.case(name)
        M = np.array(list(p.transform), np.float32).reshape(4, 4)
        for b in range(of.num_batches):
            r = SC.batch_reference(sname, p, b)
            if not r["full"]:
                continue
            xyz = of.decode_batch(b).reshape(SC.PPB, 3)[r["index"] - b * SC.PPB]
            g = of.batch(b)
            sc = np.array([g.scale_x, g.scale_y, g.scale_z]); off = np.array([g.offset_x - g.las_min_x, g.offset_y - g.las_min_y, g.offset_z - g.las_min_z])
            if r["double"]:
                f = (xyz.astype(np.float64) * sc + off).astype(np.float32)          # (the fma differs from this in rare last bits: w only to 1 ulp)
            else:
                f = (xyz.astype(np.float32).astype(np.float64) * sc.astype(np.float32).astype(np.float64) + off.astype(np.float32).astype(np.float64)).astype(np.float32)
            w = (f.astype(np.float64) @ M[3, :3].astype(np.float64) + np.float64(M[3, 3])).astype(np.float32)
            close = np.abs(w.view(np.int32).astype(np.int64) - r["depth"].astype(np.int64)) <= 4
            assert close.mean() > 0.999, (name, b, close.mean())
            checked += 1
    assert checked >= 10


def test_tie_window_holds_points_that_only_the_index_tells_apart():
    sname, of, p, _ = SC.case(SC.PICK_CASE)
    ref = SC.reference(sname, p, None)
    assert all(r["full"] for r in ref)
    pix, depth, colour, index = (np.concatenate([r[k] for r in ref]) for k in ("pix", "depth", "colour", "index"))
    px, py = SC.PICK_TIE
    w, tied = SC.pick_reference(pix, depth, colour, index, p, px, py, 0)
    assert tied > 1, "the winning depth and colour of the tie pixel is held by one point only"
    m = (pix == px + py * p.width) & (depth == depth[w]) & (colour == colour[w])
    assert len(np.unique(index[m])) == tied and index[m].min() == index[w]
    # and the frame has both occupied and empty pixels for the radius-0 picks
    occupied = np.unique(pix[pix < p.width * p.height])
    assert 0 < len(occupied) < p.width * p.height
