"""ctypes binding of tests/las_hqs_ref.c, the CPU reference of the 10-10-10 HQS method ("loop_las_hqs"): depth pass and colour
sums. Test infrastructure only. Compiled on first use into a temporary directory with the oracle Makefile's flags, in the style of
tests/oracle.py."""
from __future__ import annotations

import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

from pcrhpg24_amd._native import RenderParams, RenderStats, fb_elems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "las_hqs_ref.c")
CFLAGS = ["-O2", "-std=gnu11", "-ffp-contract=off", "-mfma", "-fPIC"]      # oracle/Makefile

_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        tmp = tempfile.mkdtemp(prefix="las_hqs_ref_")
        atexit.register(shutil.rmtree, tmp, True)
        so = os.path.join(tmp, "liblas_hqs_ref.so")
        subprocess.run(["gcc", *CFLAGS, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "oracle"), "-shared", SRC,
                        "-o", so, "-lm", "-lpthread"], check=True)
        L = C.CDLL(so)
        L.las_hqs_ref_depth.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RenderParams),
                                        C.c_void_p, C.POINTER(RenderStats)]
        L.las_hqs_ref_depth.restype = None
        L.las_hqs_ref_color.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.POINTER(RenderParams), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RenderStats)]
        L.las_hqs_ref_color.restype = None
        L.las_hqs_ref_points.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RenderParams),
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
        L.las_hqs_ref_points.restype = C.c_int64
        _lib = L
    return _lib


def _nb(batches, num_batches):
    return len(batches) if num_batches is None else num_batches


def render_depth(batches, xyz12, xyz8, xyz4, p: RenderParams, fb=None, num_batches=None):
    """The depth pass: (fb, stats). Keys f32_bits(w) << 32, payload 0."""
    fb = np.full(fb_elems(p.width, p.height), 0xFFFFFFFFFFFFFFFF, np.uint64) if fb is None else fb
    st = RenderStats()
    lib().las_hqs_ref_depth(C.addressof(batches), _nb(batches, num_batches), xyz12.ctypes.data, xyz8.ctypes.data, xyz4.ctypes.data,
                            C.byref(p), fb.ctypes.data, C.byref(st))
    return fb, st.as_dict()


def render_color(batches, xyz12, xyz8, xyz4, rgba, p: RenderParams, fb, rg=None, ba=None, num_batches=None):
    """The colour pass over the depth pass's `fb`: (rg, ba, stats)."""
    n = fb_elems(p.width, p.height)
    rg = np.zeros(n, np.uint64) if rg is None else rg
    ba = np.zeros(n, np.uint64) if ba is None else ba
    st = RenderStats()
    lib().las_hqs_ref_color(C.addressof(batches), _nb(batches, num_batches), xyz12.ctypes.data, xyz8.ctypes.data, xyz4.ctypes.data,
                            rgba.ctypes.data, C.byref(p), fb.ctypes.data, rg.ctypes.data, ba.ctypes.data, C.byref(st))
    return rg, ba, st.as_dict()


def drawn_points(batches, xyz12, xyz8, xyz4, p: RenderParams, num_batches=None, with_index=False):
    """(pixel int64, w float32) of every point the passes draw; with_index: and its point index (uint32)."""
    nb = _nb(batches, num_batches)
    cap = max(nb - 1, 0) * 65536
    pix, w = np.zeros(cap, np.int64), np.zeros(cap, np.float32)
    index = np.zeros(cap, np.uint32) if with_index else None
    n = lib().las_hqs_ref_points(C.addressof(batches), nb, xyz12.ctypes.data, xyz8.ctypes.data, xyz4.ctypes.data, C.byref(p),
                                 pix.ctypes.data, w.ctypes.data, index.ctypes.data if with_index else None, cap)
    assert n <= cap
    return (pix[:n], w[:n], index[:n]) if with_index else (pix[:n], w[:n])
