"""In-tree builds of the native libraries (no JIT cache, no pip): the .so files land next to this
file so they travel to the GPU box with the repository snapshot.

    libpcr_hip.so   hipcc --offload-arch=gfx950   csrc/pcr_api.hip (+ pcr_kernels.hip.h, pcr_gpu_encoder.hip.h, pcr_lattice.h, pcr_polygon.h, pcr_plane.h)   hot path + GPU encoder
    libpcr_host.so  g++                           csrc/pcr_encoder.cpp                     CPU encoder / generator / camera
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG_DIR)
CSRC = os.path.join(PKG_DIR, "csrc")
INCLUDE = os.path.join(ROOT, "include")

HIP_LIB = os.environ.get("PCR_HIP_LIB") or os.path.join(PKG_DIR, "libpcr_hip.so")   # override: experiment builds
HOST_LIB = os.path.join(PKG_DIR, "libpcr_host.so")

# -ffp-contract=off is part of the numeric contract: FMAs are spelled out in the sources.
# -amdgpu-sched-strategy=max-ilp: hipcc's scheduler that orders a region for instruction-level parallelism first. Same-box A/B of the
# whole library (profiles/r04_experiments.md section 10): the HQS frame -3 %, every other row within +-1 %.
HIP_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-mllvm", "-amdgpu-sched-strategy=max-ilp", "-fPIC", "-shared"]
HOST_FLAGS = ["-O2", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fPIC", "-shared"]


def _stale(target: str, sources: list[str]) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources)


def _run(cmd: list[str]) -> None:
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout)
        raise RuntimeError("build failed: " + " ".join(cmd))


def _hipcc() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: the gfx950 code object cannot be built")


def build_hip(force: bool = False) -> str:
    srcs = [os.path.join(CSRC, "pcr_api.hip"), os.path.join(CSRC, "pcr_kernels.hip.h"), os.path.join(CSRC, "pcr_gpu_encoder.hip.h"),
            os.path.join(CSRC, "pcr_codec_common.h"), os.path.join(CSRC, "pcr_lattice.h"), os.path.join(CSRC, "pcr_polygon.h"), os.path.join(CSRC, "pcr_plane.h"),
            os.path.join(INCLUDE, "pcr_hip.h"),
            os.path.join(INCLUDE, "pcr_types.h"), os.path.join(INCLUDE, "pcr_encode.h"), os.path.join(INCLUDE, "pcr_gpu_encode.h")]
    if force or _stale(HIP_LIB, srcs):
        _run([_hipcc(), *HIP_FLAGS, "-I", INCLUDE, "-I", CSRC, srcs[0], "-o", HIP_LIB])
    return HIP_LIB


def build_host(force: bool = False) -> str:
    srcs = [os.path.join(CSRC, "pcr_encoder.cpp"), os.path.join(CSRC, "pcr_codec_common.h"), os.path.join(INCLUDE, "pcr_encode.h"),
            os.path.join(INCLUDE, "pcr_types.h")]
    if force or _stale(HOST_LIB, srcs):
        _run(["g++", *HOST_FLAGS, "-I", INCLUDE, "-I", CSRC, srcs[0], "-o", HOST_LIB, "-lpthread"])
    return HOST_LIB


DIST_LIB = os.path.join(PKG_DIR, "libpcr_dist.so")
RENDER_DIST_BIN = os.path.join(PKG_DIR, "pcr_render_dist")


def build_dist(force: bool = False) -> str:
    """libpcr_dist.so (include/pcr_dist.h): the multi-GPU layer in C++ over RCCL, and its headless driver pcr_render_dist."""
    build_hip(force)
    build_host(force)
    srcs = [os.path.join(CSRC, "pcr_dist.cpp"), os.path.join(INCLUDE, "pcr_dist.h"), os.path.join(INCLUDE, "pcr_hip.h"), HIP_LIB]
    if force or _stale(DIST_LIB, srcs):
        _run([_hipcc(), "-O2", "-std=c++17", "-fPIC", "-shared", "-I", INCLUDE, "-I", CSRC, srcs[0], "-o", DIST_LIB,
              "-L", PKG_DIR, "-lpcr_hip", "-lrccl", "-Wl,-rpath,$ORIGIN"])
    dsrc = [os.path.join(CSRC, "pcr_render_dist.cpp"), DIST_LIB, HOST_LIB]
    if force or _stale(RENDER_DIST_BIN, dsrc):
        _run([_hipcc(), "-O2", "-std=c++17", "-I", INCLUDE, "-I", CSRC, dsrc[0], "-o", RENDER_DIST_BIN,
              "-L", PKG_DIR, "-lpcr_dist", "-lpcr_hip", "-lpcr_host", "-lrccl", "-lpthread", "-Wl,-rpath,$ORIGIN"])
    return DIST_LIB


RENDER_BIN = os.path.join(PKG_DIR, "pcr_render")
PREPROCESS_BIN = os.path.join(PKG_DIR, "pcr_preprocess")
DECODE_BIN = os.path.join(PKG_DIR, "pcr_decode")


def build_tools(force: bool = False) -> None:
    """C++ host adapters (csrc/pcr_methods.hpp) as headless executables: pcr_render (the reference's main.cpp flow),
    pcr_preprocess (the reference's preprocess CLI) and pcr_decode (.huffman -> .las, decoded on the GPU)."""
    build_host(force)
    build_hip(force)
    rsrc = [os.path.join(CSRC, "pcr_render.cpp"), os.path.join(CSRC, "pcr_methods.hpp"), os.path.join(CSRC, "pcr_las_reader.hpp"),
            HIP_LIB, HOST_LIB]
    if force or _stale(RENDER_BIN, rsrc):
        _run([_hipcc(), "-O2", "-std=c++17", "-I", INCLUDE, "-I", CSRC, rsrc[0], "-o", RENDER_BIN,
              "-L", PKG_DIR, "-lpcr_hip", "-lpcr_host", "-lpthread", "-Wl,-rpath,$ORIGIN"])
    dsrc = [os.path.join(CSRC, "pcr_decode.cpp"), os.path.join(CSRC, "pcr_methods.hpp"), os.path.join(CSRC, "pcr_las_reader.hpp"),
            HIP_LIB, HOST_LIB]
    if force or _stale(DECODE_BIN, dsrc):
        _run([_hipcc(), "-O2", "-std=c++17", "-I", INCLUDE, "-I", CSRC, dsrc[0], "-o", DECODE_BIN,
              "-L", PKG_DIR, "-lpcr_hip", "-lpcr_host", "-lpthread", "-Wl,-rpath,$ORIGIN"])
    psrc = [os.path.join(CSRC, "pcr_preprocess.cpp"), os.path.join(CSRC, "pcr_las_reader.hpp"), HOST_LIB, HIP_LIB]
    if force or _stale(PREPROCESS_BIN, psrc):
        _run(["g++", "-O2", "-std=c++17", "-Wall", "-I", INCLUDE, "-I", CSRC, psrc[0], "-o", PREPROCESS_BIN,
              "-L", PKG_DIR, "-lpcr_host", "-lpcr_hip", "-lpthread", "-Wl,-rpath,$ORIGIN"])


def build_all(force: bool = False) -> None:
    build_host(force)
    build_hip(force)
    build_tools(force)
    build_dist(force)


if __name__ == "__main__":
    build_all(force="--force" in sys.argv)
    print(HIP_LIB)
    print(HOST_LIB)
