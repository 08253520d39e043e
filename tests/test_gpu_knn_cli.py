"""pcr_decode --sor and HuffmanLasData.statistical_outliers / nearest_neighbors on a small constructed scene: a 60 x 60 planar grid of
spacing 10 and five strays 300 units off it (tests/knn_cases.py; tests/test_knn_cpu.py asserts from the numpy reference that with k =
8, multiplier 2 and a radius of 320 steps exactly the five strays are outliers). The rest of the batch lies outside the box the calls
pass."""
import subprocess

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import build
from tests import knn_cases as KC

pytestmark = pytest.mark.gpu

SCALE = 0.001
LO, HI = (tuple(v * SCALE for v in c) for c in KC.SOR_BOX)
RADIUS = KC.SOR_R * SCALE + 0.0002                                          # 320 lattice steps of 0.001
BOX = ["--box", *(repr(v) for v in LO + HI)]


def run(tmp_path, out, *args):
    (tmp_path / "scene.huffman").write_bytes(bytes(KC.sor_stream()))
    return subprocess.run([str(build.DECODE_BIN), str(tmp_path / "scene.huffman"), str(tmp_path / out), "--sor", *args], stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True, timeout=600)


def scene():
    """(rows of the grid, rows of the strays) among the stream's rows."""
    xyz = KC.sor_rows()
    inside = (xyz[:, 0] <= KC.SOR_BOX[1][0])
    return np.nonzero(inside & (xyz[:, 2] == 1000))[0], np.nonzero(inside & (xyz[:, 2] != 1000))[0]


@pytest.mark.parametrize("outliers", [False, True], ids=["inliers", "outliers"])
def test_sor_writes_the_grid_or_the_strays(tmp_path, outliers):
    build.build_tools()
    grid, strays = scene()
    assert len(grid) == KC.SOR_SIDE ** 2 and len(strays) == 5
    res = run(tmp_path, "out.las", str(KC.SOR_K), repr(KC.SOR_MULT), repr(RADIUS), *(["--outliers"] if outliers else []), *BOX)
    assert res.returncode == 0, res.stderr
    x, y, z, c, las = P.read_las(str(tmp_path / "out.las"))
    want = KC.sor_rows()[strays if outliers else grid]
    assert len(x) == len(want), res.stdout
    assert np.array_equal(np.stack([x, y, z], axis=1).astype(np.int64), want), "the points written are not the expected rows in the stream's order"
    an = KC.analyse(KC.sor_rows(), KC.SOR_K, KC.SOR_R, KC.SOR_BOX)
    assert (f"sor: k {KC.SOR_K}, {KC.SOR_R} lattice steps, written {len(want)}, considered {len(grid) + 5}, outliers 5, voxels {an['voxels']}, "
            f"pairs bound {an['pairs_bound']}") in res.stdout, res.stdout


def test_the_resource_returns_the_same_rows():
    import torch
    grid, strays = scene()
    r = P.Renderer(160, 90)
    try:
        data = P.HuffmanLasData.create(KC.sor_stream())
        data.load_all(r)
        assert P.radius_from_world(data.las_info(), RADIUS) == KC.SOR_R
        everything = r.ctx.read_points()
        for outliers, want in ((False, grid), (True, strays)):
            pts, rows = data.statistical_outliers(r, KC.SOR_K, KC.SOR_MULT, RADIUS, LO, HI, outliers=outliers)
            assert rows.dtype == np.int64 and np.array_equal(rows, want) and pts.tobytes() == everything[want].tobytes()
            pts2, rows2 = data.statistical_outliers(r, KC.SOR_K, KC.SOR_MULT, KC.SOR_R, KC.SOR_BOX[0], KC.SOR_BOX[1], outliers=outliers, world=False)
            assert np.array_equal(rows2, rows) and pts2.tobytes() == pts.tobytes()
        # nearest_neighbors: the reference's lists, distances in world units
        an = KC.analyse(KC.sor_rows(), 4, KC.SOR_R, KC.SOR_BOX)
        pts, rows, krows, dist = data.nearest_neighbors(r, 4, RADIUS, LO, HI)
        want_rows, want_d2 = KC.split(an["knn"])
        assert dist.dtype == torch.float64 and np.array_equal(rows.cpu().numpy(), an["rows"]) and np.array_equal(krows.cpu().numpy(), want_rows)
        assert np.array_equal(dist.cpu().numpy(), np.where(want_d2 < 0, np.inf, np.sqrt(np.maximum(want_d2, 0).astype(np.float64)) * SCALE))
        assert pts.cpu().numpy().tobytes() == everything[an["rows"]].tobytes()
    finally:
        r.ctx.close()


def test_nothing_to_write_and_a_radius_too_large_are_errors(tmp_path):
    build.build_tools()
    for args, word in (([str(KC.SOR_K), "2", repr(RADIUS), "--box", "50", "50", "50", "60", "60", "60"], "no points"),
                       ([str(KC.SOR_K), "2", "40.0", *BOX], "pcr_read_knn")):
        res = run(tmp_path, "none.las", *args)
        assert res.returncode == 1 and word in res.stderr and not (tmp_path / "none.las").exists(), res.stderr
