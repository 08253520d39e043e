"""Display resolves (pcr_resolve_*_display), the parts that need no GPU: the three entry points and the struct in the headers, the
binding tables and the cross-compiled library; the CLI's refusal of malformed --window / --edl / --edl-window before any device is
touched; the numpy reference of tests/display_ref.py against an independent formulation (squares drawn with a 64-bit minimum);
the preconditions of tests/test_gpu_display.py, from the oracle alone; and the EDL tolerance cap met by the reference itself."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import _native as N
from pcrhpg24_amd import build
from tests import display_ref as R
from tests.test_abi import declared

SYMBOLS = ("pcr_resolve_basic_display", "pcr_resolve_hqs_display", "pcr_resolve_las_display")
CAMERAS = ("closeup", "overview")


def test_entry_points_are_declared_bound_and_exported():
    for name in SYMBOLS:
        assert name in declared("pcr_hip.h") and name in N.HIP_SYMBOLS
    build.build_hip()
    lib = C.CDLL(build.HIP_LIB)
    for name in SYMBOLS:
        assert hasattr(lib, name)
    bound = N.hip_lib()
    for name in SYMBOLS:
        assert getattr(bound, name).argtypes == [C.c_void_p, C.POINTER(N.RenderParams), C.POINTER(N.DisplayOpts)]
    assert P.DisplayOpts is N.DisplayOpts
    for name in ("resolve_basic_display", "resolve_hqs_display", "resolve_las_display"):
        assert callable(getattr(P.Context, name))
    for method in (P.HuffmanMemIter, P.HuffmanHQS, P.ComputeLoopLasCUDA, P.ComputeLoopLasHQS):
        assert method.display is None


def test_struct_matches_the_header(tmp_path):
    """sizeof / offsetof as a C compiler sees include/pcr_types.h, against the ctypes mirror."""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pcr_types.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %d %d\\n", sizeof(pcr_display_opts), offsetof(pcr_display_opts, window),\n'
                   'offsetof(pcr_display_opts, edl_window), offsetof(pcr_display_opts, edl_strength), offsetof(pcr_display_opts, reserved),\n'
                   'PCR_DISPLAY_MAX_WINDOW, PCR_DISPLAY_MAX_EDL_WINDOW); return 0; }\n')
    subprocess.run(["gcc", "-I", build.INCLUDE, str(src), "-o", str(tmp_path / "layout")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "layout")], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert got == [16, 0, 4, 8, 12, 4, 2]
    assert [C.sizeof(N.DisplayOpts)] + [getattr(N.DisplayOpts, f).offset for f, _ in N.DisplayOpts._fields_] == got[:5]
    assert [f for f, _ in N.DisplayOpts._fields_] == ["window", "edl_window", "edl_strength", "reserved"]
    assert N.DisplayOpts._fields_[2][1] is C.c_float


# ---- the CLI -----------------------------------------------------------------------------------------------------------------
NO_DEVICE = dict(os.environ, HIP_VISIBLE_DEVICES="-1")


@pytest.mark.parametrize("args", [["--window", "5"], ["--window", "-1"], ["--edl", "nan"], ["--edl-window", "3"],
                                  ["--window", "two"], ["--edl", "-0.5"], ["--edl", "inf"], ["--edl", "0.1x"],
                                  ["--edl", "0.001", "--edl-window", "0"], ["--edl-window", "1"], ["--window"]])
def test_render_cli_refuses_malformed_display_options_before_it_creates_a_context(tmp_path, args):
    build.build_tools()
    # (the input does not exist and HIP sees no device: either would be the message if the tool got that far)
    res = subprocess.run([build.RENDER_BIN, str(tmp_path / "missing.huffman"), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=120, env=NO_DEVICE)
    assert res.returncode == 2 and res.stderr.strip() and res.stdout == ""
    assert "pcr_create" not in res.stderr and "missing.huffman" not in res.stderr


# ---- the helper against an independent formulation -------------------------------------------------------------------------------
def test_min_filter_of_the_frame_is_the_frame_of_squares():
    """The identity the feature rests on: drawing every point the oracle's trace lists as a clipped (2w+1)^2 square with a 64-bit
    minimum gives the minimum of the oracle's finished frame over each pixel's window."""
    W, H = 320, 200
    p, fb = R.basic_frame("closeup", W, H)
    pix, depth, colour = R.oracle_file().trace_points(p)
    assert len(pix) > 100_000
    assert np.array_equal(R.splat_squares(pix, depth, colour, W, H, 0).ravel(), fb[:W * H]), "the trace does not rebuild the frame itself"
    for w in R.WINDOWS:
        assert np.array_equal(R.splat_squares(pix, depth, colour, W, H, w), R.dilate(fb, W, H, w)), w


# ---- preconditions of the GPU cases ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", R.SIZES)
@pytest.mark.parametrize("cam", CAMERAS)
def test_every_offset_of_the_window_decides_some_pixel(cam, size):
    """For window 1, 2 and 4 each of the (2w+1)^2 offsets is, at some pixel, the only one that holds the minimum: a kernel that
    leaves an offset out, or reads it from the wrong side, changes a pixel. And dilation both fills empty pixels and replaces
    drawn ones."""
    W, H = size
    p, fb = R.basic_frame(cam, W, H)
    f = fb[:W * H].reshape(H, W)
    for w in R.WINDOWS:
        D = R.dilate(fb, W, H, w)
        pad = R._padded(f, w, R.EMPTY)
        holds = {o: R.shifted(pad, w, o[0], o[1], H, W) == D for o in R.offsets(w)}
        count = sum(h.astype(np.int32) for h in holds.values())
        unique = (count == 1) & (D != R.EMPTY)
        missing = [o for o, h in holds.items() if not (h & unique).any()]
        assert not missing, (cam, size, w, missing)
        assert ((f == R.EMPTY) & (D != R.EMPTY)).any(), "dilation fills no empty pixel"
        assert ((f != R.EMPTY) & (D < f)).any(), "dilation replaces no drawn pixel"


@pytest.mark.parametrize("size", R.SIZES)
@pytest.mark.parametrize("cam", CAMERAS)
def test_hqs_windows_hold_accepted_and_rejected_neighbours(cam, size):
    """Some pixels average more than one neighbour while at least one drawn neighbour fails the 1 % test: neither `all` nor
    `own pixel only` passes for the test's inputs."""
    W, H = size
    p, fb, rg, ba = R.hqs_frame(cam, W, H)
    for w in (1, 4):
        _, _, _, accepted, rejected = R.hqs_sums(p, fb, rg, ba, w)
        both = int(((accepted > 1) & (rejected >= 1)).sum())
        assert both > 0, (cam, size, w)


@pytest.mark.parametrize("size", R.SIZES)
@pytest.mark.parametrize("cam", CAMERAS)
def test_edl_shades_most_drawn_pixels_and_the_reference_meets_its_own_cap(cam, size):
    """At least half of the drawn pixels have a response > 0, and the tolerance the GPU test allows is met by the formula itself:
    evaluated in np.float32 it differs from the float64 image in at most 1 % of the drawn pixels, by 1 per channel."""
    W, H = size
    p, fb = R.basic_frame(cam, W, H)
    for w in (0, 2):
        img, D = R.basic_image(p, fb, w)
        drawn = int((D != R.EMPTY).sum())
        assert drawn > 0
        for e in R.EDL_WINDOWS:
            for s in R.EDL_STRENGTHS:
                ref, response = R.edl(img, D, e, s)
                assert 2 * int((response > 0).sum()) >= drawn, (cam, size, w, e)
                assert (response[D == R.EMPTY] == 0).all() and np.array_equal(ref[D == R.EMPTY], img[D == R.EMPTY])
                assert not (ref[D != R.EMPTY] >> np.uint32(24)).any()
                single, _ = R.edl(img, D, e, s, dtype=np.float32)
                R.edl_check(single, ref, response, D)


def test_zero_opts_reference_is_the_plain_resolve():
    from tests import oracle
    p, fb = R.basic_frame("closeup", 67, 19)
    assert np.array_equal(R.basic_image(p, fb, 0)[0].ravel(), oracle.resolve_basic(p, fb))
    p, fb, rg, ba = R.hqs_frame("closeup", 67, 19)
    assert np.array_equal(R.hqs_image(p, fb, rg, ba, 0)[0].ravel(), oracle.resolve_hqs(p, fb, rg, ba))
