"""pcr_decode --dtm / --height on the `town` stream of tests/ground_cases.py against the Python resource (HuffmanLasData.
ground_model / points_by_height), which tests/test_gpu_ground.py ties to the numpy reference through the calls beneath both."""
import os
import subprocess

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import build
from tests import ground_cases as GC

pytestmark = pytest.mark.gpu

PMF = dict(slope=0.02, max_window=17.0, initial_distance=0.06, max_distance=0.235)     # windows of 3, 5, 9, 17 cells of 1 m
PMF_ARGS = ["--slope", "0.02", "--max-window", "17", "--initial", "0.06", "--max-distance", "0.235"]


def run(*cmd):
    res = subprocess.run([str(c) for c in cmd], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    return res


def read_asc(path):
    lines = open(path).read().split("\n")
    head = dict((k, float(v)) for k, v in (l.split() for l in lines[:6]))
    rows = np.array([[float(v) for v in l.split()] for l in lines[6:] if l])
    return head, rows


@pytest.fixture(scope="module")
def town(tmp_path_factory):
    build.build_tools()
    path = tmp_path_factory.mktemp("ground_cli") / "town.huffman"
    path.write_bytes(bytes(GC.stream("town")))
    r = P.Renderer(160, 90)
    las = P.HuffmanLasData.create(bytes(GC.stream("town")))
    las.load_all(r)
    yield path, r, las
    r.ctx.close()


def test_cli_dtm_equals_ground_model(town, tmp_path):
    path, r, las = town
    info = las.las_info()
    gp = P.ground_params_from_world(info, 1.0, **PMF)
    assert gp.radii == (1, 2, 4, 8) and gp.thresholds == (60, 100, 140, 220)
    height, classes, grid = las.ground_model(r, 1.0, **PMF)
    assert (grid.origin_x, grid.origin_y, grid.cell) == (0, 0, 1000) and grid.width >= 64 and grid.height >= 64
    res = run(build.DECODE_BIN, path, tmp_path / "dtm.asc", "--dtm", "1.0", *PMF_ARGS)
    head, rows = read_asc(tmp_path / "dtm.asc")
    assert (head["ncols"], head["nrows"], head["cellsize"], head["NODATA_value"]) == (grid.width, grid.height, 1.0, -9999.0)
    assert (head["xllcorner"], head["yllcorner"]) == (grid.origin_x * info.scale[0] + info.offset[0], grid.origin_y * info.scale[1] + info.offset[1])
    want = height.cpu().numpy()[::-1]                                       # rows from north to south
    want = np.where(np.isnan(want), -9999.0, want)
    assert rows.shape == want.shape and rows.tobytes() == np.ascontiguousarray(want).tobytes()
    st = r.ctx.ground_stats
    assert st["cells_nonground"] > 0 and st["cells_empty"] >= 48 and st["fill_rounds"] >= 2
    assert f"ground {st['cells_ground']}, non-ground {st['cells_nonground']}," in res.stdout and f"in {st['fill_rounds']} rounds" in res.stdout
    cls = classes.cpu().numpy()
    assert ((cls == P.CELL_GROUND).sum(), (cls == P.CELL_NONGROUND).sum()) == (st["cells_ground"], st["cells_nonground"])
    # a box: its x and y range carries the cells, its z range clips the points
    res = run(build.DECODE_BIN, path, tmp_path / "part.asc", "--dtm", "1.0", *PMF_ARGS, "--box", "10", "10", "0", "39.999", "29.999", "9")
    head, rows = read_asc(tmp_path / "part.asc")
    assert rows.shape == (20, 30) and (head["xllcorner"], head["yllcorner"]) == (10.0, 10.0)


@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalize"])
def test_cli_height_equals_points_by_height(town, tmp_path, normalize):
    path, r, las = town
    xyz, pts, h = las.points_by_height(r, 1.0, 2.0, 20.0, normalize=normalize, **PMF)
    want = pts.cpu().numpy()
    assert len(want) >= 1000 and h.cpu().numpy().min() >= 2.0 - 1e-9 and h.cpu().numpy().max() <= 20.0 + 1e-9
    if normalize:
        assert np.array_equal(want[:, 2], np.rint(h.cpu().numpy() / 0.001).astype(np.int32)) and np.array_equal(xyz[:, 2].cpu().numpy(), h.cpu().numpy())
    out = tmp_path / "veg.las"
    res = run(build.DECODE_BIN, path, out, "--height", "1.0", "2", "20", *(["--normalize"] if normalize else []), *PMF_ARGS)
    x, y, z, c, _ = P.read_las(str(out))
    assert len(x) == len(want), res.stdout
    assert np.array_equal(x, want[:, 0]) and np.array_equal(y, want[:, 1]) and np.array_equal(z, want[:, 2])
    assert np.array_equal(c.astype(np.uint32), want[:, 3].view(np.uint32))
    assert f"selected {len(want)}" in res.stdout and "height: 2000 .. 20000 z steps" in res.stdout
    st = r.ctx.height_stats
    assert st["points_selected"] == len(want) and st["batches_decoded"] == 2
    # the stream's integers instead of world units
    m = P.box_from_world(las.las_info(), tuple(las.las_info().min), tuple(las.las_info().max))
    ipts, ih = las.points_by_height(r, 1.0, 2000, 20000, lo=tuple(m.min), hi=tuple(m.max), normalize=normalize, world=False, **PMF)
    assert np.array_equal(ipts.cpu().numpy(), want) and np.array_equal(ih.cpu().numpy(), np.rint(h.cpu().numpy() / 0.001).astype(np.int32))


@pytest.mark.parametrize("args", [["--dtm"], ["--dtm", "0"], ["--dtm", "x"], ["--dtm", "1", "--normalize"], ["--dtm", "1", "--slope"], ["--dtm", "1", "--slope", "-1"],
                                  ["--dtm", "1", "--slope", "1", "--slope", "2"], ["--height", "1"], ["--height", "1", "2"], ["--height", "1", "a", "3"],
                                  ["--height", "1", "2", "3", "--normalize", "--normalize"], ["--height", "1", "2", "3", "--box", "1", "2"]])
def test_cli_refuses_malformed_ground_options_before_it_creates_a_context(tmp_path, args):
    build.build_tools()
    out = tmp_path / "out.asc"
    res = subprocess.run([build.DECODE_BIN, str(tmp_path / "missing.huffman"), str(out), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert res.returncode == 2 and res.stderr.startswith("usage: pcr_decode") and "--dtm CELL" in res.stderr and "--height CELL LO HI" in res.stderr
    assert "pcr_create" not in res.stderr and not out.exists()
