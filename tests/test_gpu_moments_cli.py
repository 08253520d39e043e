"""pcr_decode --normals: the PLY it writes equals HuffmanLasData.normals of the same arguments -- the world coordinates and the
colours exactly, the normals and the curvature as the single-precision rounding of the float64 values -- and a malformed option
prints the usage and exits non-zero."""
import subprocess

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import build
from tests import moments_cases as MC

pytestmark = pytest.mark.gpu

PLY_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("red", "u1"), ("green", "u1"), ("blue", "u1"),
                      ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("curvature", "<f4")])
HEADER = ("ply\nformat binary_little_endian 1.0\ncomment pcr_decode --normals\nelement vertex {n}\nproperty double x\nproperty double y\n"
          "property double z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty float nx\nproperty float ny\n"
          "property float nz\nproperty float curvature\nend_header\n")


def read_ply(path):
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    n = int(raw[:end].split(b"element vertex ")[1].split(b"\n")[0])
    assert raw[:end].decode() == HEADER.format(n=n) and len(raw) == end + n * PLY_DTYPE.itemsize and PLY_DTYPE.itemsize == 43
    return np.frombuffer(raw[end:], PLY_DTYPE)


@pytest.mark.parametrize("args,min_count,boxed", [(["3"], 3, False), ([], 3, False), (["1"], 1, False), (["3", "--box", "0", "0", "0", "6", "20", "20"], 3, True)],
                         ids=["min3", "default", "min1", "box"])
def test_normals_ply_equals_the_resource(tmp_path, args, min_count, boxed):
    import torch
    build.build_tools()
    image = MC.stream("facets")
    (tmp_path / "facets.huffman").write_bytes(bytes(image))
    radius = 0.0505                                                         # 50 lattice steps of 0.001
    res = subprocess.run([str(build.DECODE_BIN), str(tmp_path / "facets.huffman"), str(tmp_path / "out.ply"), "--normals", repr(radius), *args],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    ply = read_ply(tmp_path / "out.ply")
    r = P.Renderer(160, 90)
    try:
        data = P.HuffmanLasData.create(image)
        data.load_all(r)
        info = data.las_info()
        assert P.radius_from_world(info, radius) == MC.FACETS_R
        lo, hi = ((0.0, 0.0, 0.0), (6.0, 20.0, 20.0)) if boxed else (None, None)
        pts, normals, curvature = data.normals(r, radius, min_count, lo, hi)
        assert normals.dtype == torch.float64 and tuple(normals.shape) == (len(pts), 3) and curvature.dtype == torch.float64
        st = dict(r.ctx.moments_stats)
        pts, normals, curvature = pts.cpu().numpy(), normals.cpu().numpy(), curvature.cpu().numpy()
        default = data.normals(r, radius, lo=lo, hi=hi)                     # min_count = 3
        if min_count == 3:
            assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(default, (pts, normals, curvature)))
        if not boxed:                                                       # in lattice steps, no clip: every row lies in the header's box
            steps = data.normals(r, MC.FACETS_R, min_count, world=False)
            assert np.array_equal(steps[0].cpu().numpy(), pts) and np.array_equal(steps[1].cpu().numpy(), normals)
    finally:
        r.ctx.close()
    cls = MC.facets_classes(pts[:, :3])
    want_n = MC.PPB - (3 if min_count == 3 else 0)
    assert len(ply) == len(pts) and (boxed or len(pts) == want_n), res.stdout
    assert boxed == (len(pts) < 30000) and cls["horizontal"].sum() == 10000 and cls["wall"].sum() == 10000
    scale, offset = np.array(tuple(info.scale)), np.array(tuple(info.offset))
    xyz = pts[:, :3].astype(np.float64) * scale + offset
    colour = pts[:, 3].view(np.uint32)
    assert np.array_equal(np.stack([ply["x"], ply["y"], ply["z"]], axis=1), xyz), "the world coordinates differ"
    assert np.array_equal(ply["red"], colour & 255) and np.array_equal(ply["green"], (colour >> 8) & 255) and np.array_equal(ply["blue"], (colour >> 16) & 255)
    got = np.stack([ply["nx"], ply["ny"], ply["nz"]], axis=1)
    assert got.dtype == np.float32 and got.tobytes() == normals.astype(np.float32).tobytes(), "the normals are not the f32 rounding"
    assert ply["curvature"].tobytes() == curvature.astype(np.float32).tobytes(), "the curvature is not the f32 rounding"
    assert (got[cls["horizontal"]] == np.array([0, 0, 1], np.float32)).all() and (got[cls["wall"]] == np.array([1, 0, 0], np.float32)).all()
    assert (ply["curvature"][cls["horizontal"]] == 0).all() and (ply["curvature"][cls["wall"]] == 0).all()
    assert (f"normals: {MC.FACETS_R} lattice steps, written {len(pts)}, considered {st['points_considered']}, below min count {st['points_sparse']}, "
            f"voxels {st['voxels']}, pairs bound {st['pairs_bound']}") in res.stdout, res.stdout


@pytest.mark.parametrize("args", [["--normals"], ["--normals", "x"], ["--normals", "0.05", "-1"], ["--normals", "0.05", "3", "--sparse"],
                                  ["--normals", "0.05", "--box", "0", "0", "0", "1", "1"]])
def test_a_malformed_option_prints_the_usage(tmp_path, args):
    build.build_tools()
    (tmp_path / "facets.huffman").write_bytes(bytes(MC.stream("facets")))
    res = subprocess.run([str(build.DECODE_BIN), str(tmp_path / "facets.huffman"), str(tmp_path / "out.ply"), *args], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True, timeout=120)
    assert res.returncode == 2 and res.stderr.startswith("usage: pcr_decode") and "--normals R [MINCOUNT]" in res.stderr
    assert not (tmp_path / "out.ply").exists()


def test_nothing_to_write_and_a_radius_too_large_are_errors(tmp_path):
    build.build_tools()
    (tmp_path / "facets.huffman").write_bytes(bytes(MC.stream("facets")))
    for args, word in ((["0.0505", "100000"], "no points"), (["40.0"], "pcr_read_local_moments")):
        res = subprocess.run([str(build.DECODE_BIN), str(tmp_path / "facets.huffman"), str(tmp_path / "none.ply"), "--normals", *args],
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert res.returncode == 1 and word in res.stderr and not (tmp_path / "none.ply").exists(), res.stderr
