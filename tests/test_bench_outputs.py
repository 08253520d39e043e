"""bench.py's plain run, --full and --dump-outputs: the options parse, the dump holds float arrays within 64 MB, and (on the
GPU) a short plain run prints the headline line and dumps the image its last timed step resolved, equal to the CPU oracle's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse_args()


def test_plain_is_the_default(monkeypatch):
    a = _args(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = _args(monkeypatch, "--full", "--dump-outputs", "out")
    assert a.full is True and a.dump_outputs == "out"
    with pytest.raises(SystemExit) as e:           # every help string formats
        _args(monkeypatch, "--help")
    assert e.value.code == 0


def _stats():
    return {"batches_total": 7, "batches_culled": 2, "points_iterated": 123456, "batches_double": 0}


def test_dump_outputs_whole_image(tmp_path):
    w, h = 64, 32
    rgba = np.random.default_rng(1).integers(0, 2**32, w * h, dtype=np.uint64).astype(np.uint32)
    bench.dump_outputs(str(tmp_path), rgba, w, h, _stats())
    img = np.load(tmp_path / "rgba.npy")
    assert img.dtype == np.float32 and img.shape == (h, w, 4)
    assert np.array_equal(img.astype(np.uint8).reshape(-1).view(np.uint32), rgba)
    st = np.load(tmp_path / "stats.npy")
    assert st.dtype == np.float64 and st.tolist() == [7, 2, 123456, 0]


def test_dump_outputs_samples_a_large_image(tmp_path):
    w = h = 4096
    rgba = np.arange(w * h, dtype=np.uint32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), rgba, w, h, _stats())
        assert sum(os.path.getsize(tmp_path / d / f) for f in os.listdir(tmp_path / d)) <= 64 << 20
    a, b = (np.load(tmp_path / d / "rgba_sample_index.npy") for d in ("a", "b"))
    assert a.dtype == np.float64 and np.array_equal(a, b) and np.all(np.diff(a) > 0)      # the same fixed sample every run
    s = np.load(tmp_path / "a" / "rgba_sample.npy")
    assert s.dtype == np.float32 and np.array_equal(s.astype(np.uint8).reshape(-1).view(np.uint32), rgba[a.astype(np.int64)])


@pytest.mark.gpu
def test_plain_run_dumps_its_last_step(tmp_path):
    import pcrhpg24_amd as P
    from tests import oracle

    n, w, h, steps = bench.CHUNK, 1920, 1080, 5          # one chunk: 100 batches
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2",
                        "--preroll", "0", "--points", str(n), "--dump-outputs", str(out)],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for key, typ in (("metric", str), ("value", float), ("unit", str), ("higher_is_better", bool), ("dtype", str), ("ms_per_step", float)):
        assert isinstance(line[key], typ), key
    assert line["steps"] == steps and line["config"]["points_per_step"] > 0
    assert line["roofline"] is None and line["secondary"] is None and line["cpu_baseline"] is None     # --full only

    image, _ = P.synth_encode(n, 0x5EED, 0, n, bench.CHUNK, 4)
    p = bench.camera(P, "overview", w, h)
    p.lod_percent, p.enable_frustum_culling = 100, 0
    ofb, ost = oracle.OracleFile(image.view()).render_basic(p, nthreads=4)
    img = np.load(out / "rgba.npy")
    assert img.dtype == np.float32 and img.shape == (h, w, 4)
    assert np.array_equal(img.astype(np.uint8).reshape(-1).view(np.uint32), oracle.resolve_basic(p, ofb))
    assert np.load(out / "stats.npy").tolist() == [ost[k] for k in bench.STATS_FIELDS]
