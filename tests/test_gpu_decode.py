"""pcr_decode_points / pcr_read_points: the loaded stream back to points, on the GPU, against the oracle's decoder.

Every case runs for a context loaded with PCR_LAYOUT_WORDS, PCR_LAYOUT_POINT_WINDOWS and PCR_LAYOUT_BOTH (there by both
kernels: pcr_set_render_variant), AFTER one rendered frame -- the frame that releases what only the load-time transcode reads
(raw words, lane words, int8 lengths, cluster prefix, file-order colours) -- and case 1 also before any frame. All
comparisons are exact and cover every point of every batch.

Colours: the record holds 0x00BBGGRR. oracle.decode_bc1 returns exactly that; oracle.decode_bc7 also returns the block's alpha
in bits 24..31, which the record has no room for and is masked off here."""
import ctypes as C
import subprocess
import time

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import build
from tests import oracle, scenes

pytestmark = pytest.mark.gpu

PPB = 65536
PCR_E_ARG = -1
GOLDEN = ["config1", "ref_packed_batch", "ref_packed_lowentropy", "ref_packed_bc7"]
LAYOUTS = {"words": P.Context.LAYOUT_WORDS, "point_windows": P.Context.LAYOUT_POINT_WINDOWS, "both": P.Context.LAYOUT_BOTH}


def golden(name):
    import os
    return open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".huffman"), "rb").read()


@pytest.fixture(params=list(LAYOUTS))
def ctx(request):
    c = P.Context(0)
    c.set_stream_layout(LAYOUTS[request.param])
    c.set_image_size(160, 90)
    c.layout_name = request.param
    yield c
    c.close()


def one_frame(c):
    """A frame over the whole stream (the HQS depth pass: it draws BC1 and BC7 streams alike)."""
    p = scenes.with_flags(P.camera_orbit(-0.15, -0.57, 1500.0, (500.0, 500.0, 40.0), 160, 90), lod_percent=100, cull=0)
    c.clear(); c.render_hqs_depth(p); c.synchronize()


def load(c, image, frame=True, first=0, count=None):
    f = P.HuffmanFile(image)
    count = f.numBatches - first if count is None else count
    if c.batches_loaded:
        c.stream_unload()
    c.stream_begin(f.header(first, count), first)
    for i in range(count):
        c.upload_batch(i, f.blob(first + i))
    if first + count < f.numBatches:
        c.upload_tail(*f.head_words(first + count))
    if frame:
        before = c.resident_bytes
        one_frame(c)
        assert c.resident_bytes < before, "the first frame after the last upload releases the load-time buffers"
    return f


def decode(c, first=0, count=None):
    """read_points of the range; a context that holds both layouts decodes with both kernels, which have to agree."""
    if c.layout_name != "both":
        return c.read_points(first, count)
    outs = []
    for v in (P.Context.VARIANT_WORDS, P.Context.VARIANT_POINT_WINDOWS):
        c.set_render_variant(v)
        outs.append(c.read_points(first, count))
    c.set_render_variant(P.Context.VARIANT_AUTO)
    assert np.array_equal(outs[0], outs[1]), "the two layouts of one stream decode to different points"
    return outs[0]


def xyz_of(pts):
    return np.stack([pts["x"], pts["y"], pts["z"]], axis=1)


def oracle_xyz(of, b):
    return of.decode_batch(b).reshape(PPB, 3)


def oracle_colors(of, b):
    bc7 = int(of.s.color_format) == 7
    col = np.ctypeslib.as_array(C.cast(of.s.colors, C.POINTER(C.c_uint8)), (of.num_batches * (PPB if bc7 else PPB // 2),))
    ptr = col.ctypes.data
    lib = oracle.lib()
    fn = lib.pcr_oracle_decode_bc7 if bc7 else lib.pcr_oracle_decode_bc1
    return np.fromiter((fn(b * PPB + i, ptr) & 0xFFFFFF for i in range(PPB)), np.uint32, PPB)


def check_against_oracle(pts, of, first=0, count=None, colors=True):
    count = of.num_batches - first if count is None else count
    assert len(pts) == count * PPB
    for i in range(count):
        got = pts[i * PPB:(i + 1) * PPB]
        bad = np.nonzero((xyz_of(got) != oracle_xyz(of, first + i)).any(axis=1))[0]
        assert bad.size == 0, f"batch {first + i}: {bad.size} points differ from the oracle's, first at {bad[:4]}"
        if colors:
            badc = np.nonzero(got["color"] != oracle_colors(of, first + i))[0]
            assert badc.size == 0, f"batch {first + i}: {badc.size} colours differ from the oracle's, first at {badc[:4]}"


# ---- 1. the committed streams -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDEN)
@pytest.mark.parametrize("frame", [True, False], ids=["after_frame", "before_any_frame"])
def test_golden_streams_decode_to_the_oracles_points(ctx, name, frame):
    image = golden(name)
    of = oracle.OracleFile(image)
    load(ctx, image, frame=frame)
    check_against_oracle(decode(ctx), of)


# ---- 2. round trip without the oracle ---------------------------------------------------------------------------------------------
N_RT = 300_000


def synth_rt():
    return P.synth_points(N_RT, scenes.SEED, 0, N_RT)


def padded(a, n):
    return np.concatenate([a, np.full(n - len(a), a[-1], a.dtype)])


def test_round_trip_unsorted_pad_tails_returns_the_input(ctx):
    x, y, z, c = synth_rt()
    image, st = P.encode_points(x, y, z, c, P.synth_las_info(N_RT), morton_sort=False, pad_tails=True, nthreads=2)
    load(ctx, image.view())
    pts = decode(ctx)
    assert len(pts) == 327_680 == st["num_points"]
    want = np.stack([padded(a, len(pts)) for a in (x, y, z)], axis=1)
    bad = np.nonzero((xyz_of(pts) != want).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} of {len(pts)} points differ from the input, first at {bad[:4]}"


def test_round_trip_sorted_pad_tails_returns_the_input_as_a_multiset(ctx):
    x, y, z, c = synth_rt()
    image, _ = P.encode_points(x, y, z, c, P.synth_las_info(N_RT), morton_sort=True, pad_tails=True, nthreads=2)
    load(ctx, image.view())
    got = xyz_of(decode(ctx))
    want = np.stack([padded(a, len(got)) for a in (x, y, z)], axis=1)
    got = got[np.lexsort((got[:, 2], got[:, 1], got[:, 0]))]
    want = want[np.lexsort((want[:, 2], want[:, 1], want[:, 0]))]
    assert np.array_equal(got, want)


# ---- 3. the reference's default stream: garbage tails included ------------------------------------------------------------------------
def test_reference_default_stream_equals_the_oracle_garbage_included(ctx):
    x, y, z, c = synth_rt()
    image, _ = P.encode_points(x, y, z, c, P.synth_las_info(N_RT), morton_sort=False, pad_tails=False, nthreads=2)
    of = oracle.OracleFile(image.view())
    load(ctx, image.view())
    pts = decode(ctx)
    check_against_oracle(pts, of)
    want = np.stack([padded(a, len(pts)) for a in (x, y, z)], axis=1)
    garbage = int((xyz_of(pts) != want).any(axis=1).sum())
    print(f"points that differ from the input (SURVEY B.4 tail artefact): {garbage} of {len(pts)}")
    assert garbage > 0, "the tail artefact was not exercised"


# ---- 4. streams on the checked path (built as tests/test_gpu_edge_cases.py builds them) --------------------------------------------
def las_for(lo, hi, scale=0.001):
    las = P.LasInfo()
    for k in range(3):
        las.scale[k] = scale; las.offset[k] = 0.0; las.min[k] = lo[k] * scale; las.max[k] = hi[k] * scale
    return las


@pytest.mark.parametrize("hop_bits", [30, 20])
def test_wide_table_values(ctx, hop_bits):
    """(The packed entry's real limit is 2^21, with -2^21 as its sentinel: the `limits` stream of tests/test_gpu_decoder.py sits on it.)"""
    rng = np.random.default_rng(21)
    n = 65536 * 2
    hop = np.where(np.arange(n) % 2 == 0, 0, 1 << hop_bits).astype(np.int64)
    x = (hop + rng.integers(0, 3, n)).astype(np.int32)
    y = rng.integers(0, 2000, n).astype(np.int32)
    z = rng.integers(0, 50, n).astype(np.int32)
    c = rng.integers(0, 1 << 24, n).astype(np.uint32)
    image, st = P.encode_points(x, y, z, c, las_for((0, 0, 0), (1 << 30, 2000, 50)), morton_sort=False, nthreads=2)
    of = oracle.OracleFile(image.view())
    tv = np.ctypeslib.as_array(C.cast(of.s.dt_values, C.POINTER(C.c_int32)), (4096,))
    tl = np.ctypeslib.as_array(C.cast(of.s.dt_cwlen, C.POINTER(C.c_int32)), (4096,))
    in_table = tv[tl > 0].astype(np.int64)
    if hop_bits == 30:
        assert (np.abs(in_table) >= 1 << 25).any(), "the stream must contain in-table values far outside the packed entry"
    else:
        for v in ((1 << 20) - 1, 1 << 20, -(1 << 20), -(1 << 20) - 1):
            assert (in_table == v).any(), f"the stream must contain the in-table value {v}"
    load(ctx, image.view())
    check_against_oracle(decode(ctx), of)


def test_escape_heavy_stream(ctx):
    x, y, z, c, las = scenes.random_points(131072, seed=3)
    image, st = P.encode_points(x, y, z, c, las, morton_sort=True, nthreads=2)
    assert st["escaped_symbols"] > 6144 * st["num_batches"]
    of = oracle.OracleFile(image.view())
    load(ctx, image.view())
    check_against_oracle(decode(ctx), of)


def test_batches_that_fall_apart_into_clusters(ctx):
    rng = np.random.default_rng(77)
    n = 300_000
    centres = np.array([[50_000, 60_000, 2_000], [900_000, 80_000, 9_000], [120_000, 950_000, 4_000], [880_000, 900_000, 1_000], [500_000, 500_000, 30_000]])
    which = rng.integers(0, len(centres), n)
    xyz = centres[which] + rng.normal(0, [6_000, 6_000, 800], (n, 3))
    x, y, z = (np.clip(xyz[:, k], 0, 1_000_000).astype(np.int32) for k in range(3))
    c = rng.integers(0, 1 << 24, n, dtype=np.int64).astype(np.uint32)
    image, st = P.encode_points(x, y, z, c, las_for((0, 0, 0), (1_000_000, 1_000_000, 40_000)), morton_sort=True, nthreads=2)
    of = oracle.OracleFile(image.view())
    load(ctx, image.view())
    check_against_oracle(decode(ctx), of)


# ---- 5. ranges and errors -------------------------------------------------------------------------------------------------------------
def test_ranges(ctx):
    image, _ = scenes.synth_stream(600_000)
    of = oracle.OracleFile(image.view())
    load(ctx, image.view())
    nb = of.num_batches
    assert nb == 10
    check_against_oracle(decode(ctx, 3, 1), of, 3, 1)
    check_against_oracle(decode(ctx, 3, -1), of, 3, nb - 3, colors=False)
    assert len(ctx.read_points(nb, None)) == 0 and len(ctx.read_points(2, 0)) == 0          # count == 0 succeeds


def test_two_shards_concatenate_to_the_single_contexts_output(ctx):
    image, _ = scenes.synth_stream(600_000)
    f = load(ctx, image.view())
    whole = decode(ctx)
    half = f.numBatches // 2
    parts = []
    for first, count in ((0, half), (half, f.numBatches - half)):
        load(ctx, image.view(), first=first, count=count)           # batch_index_base = first; the first shard carries the follower's head words
        parts.append(decode(ctx))
    assert np.array_equal(np.concatenate(parts), whole)


def test_errors_are_pcr_e_arg_with_a_message(ctx):
    import torch
    lib, h = ctx.lib, ctx.h
    buf = torch.empty((2 * PPB + 1, 4), dtype=torch.int32, device=f"cuda:{ctx.device}")
    host = np.empty(2 * PPB, P.POINT_DTYPE)

    def refused(rc):
        assert rc == PCR_E_ARG
        assert (lib.pcr_last_error(h) or b"") != b""

    refused(lib.pcr_decode_points(h, 0, 1, C.c_void_p(buf.data_ptr()), 2 * PPB))           # no stream loaded
    refused(lib.pcr_read_points(h, 0, 1, host.ctypes.data, 2 * PPB))
    image, _ = scenes.synth_stream(600_000)
    load(ctx, image.view())
    nb = ctx.batches_loaded
    for entry, dst in ((lib.pcr_decode_points, buf.data_ptr()), (lib.pcr_read_points, host.ctypes.data)):
        refused(entry(h, nb - 1, 2, C.c_void_p(dst), 2 * PPB))                              # a range outside the resident batches
        refused(entry(h, -1, 1, C.c_void_p(dst), 2 * PPB))
        refused(entry(h, nb + 1, -1, C.c_void_p(dst), 2 * PPB))
        refused(entry(h, 0, 2, C.c_void_p(dst), 2 * PPB - 1))                               # a capacity below count * 65536
        refused(entry(h, 0, 1, None, 2 * PPB))                                              # NULL
        assert entry(h, 0, 0, None, 0) == 0                                                 # count == 0: a no-op that succeeds
    refused(lib.pcr_decode_points(h, 0, 1, C.c_void_p(buf.data_ptr() + 4), 2 * PPB))        # not 16-byte aligned
    refused(lib.pcr_read_points(h, 0, 1, C.c_void_p(host.ctypes.data + 2), PPB))            # not aligned for a pcr_point
    # a refused call leaves the context usable
    of = oracle.OracleFile(image.view())
    check_against_oracle(decode(ctx, 0, 1), of, 0, 1)


def test_async_upload_refuses_a_range_past_the_resident_batches(ctx):
    image, _ = scenes.synth_stream(600_000)
    f = P.HuffmanFile(image.view())
    of = oracle.OracleFile(image.view())
    ctx.stream_begin(f.header(), 0)
    ctx.set_async_upload(True)
    try:
        ctx.upload_batches(0, [f.blob(b) for b in range(4)])
        deadline = time.time() + 60
        while ctx.batches_resident < 3 and time.time() < deadline:
            time.sleep(0.01)
        res = ctx.batches_resident
        assert res == 3, "the last arrived batch of an incomplete stream is not resident"
        host = np.empty(4 * PPB, P.POINT_DTYPE)
        assert ctx.lib.pcr_read_points(ctx.h, 0, res + 1, host.ctypes.data, 4 * PPB) == PCR_E_ARG
        assert (ctx.lib.pcr_last_error(ctx.h) or b"") != b""
        check_against_oracle(decode(ctx, 0, None), of, 0, res, colors=False)
        for b0 in range(4, f.numBatches, 3):
            ctx.upload_batches(b0, [f.blob(b) for b in range(b0, min(b0 + 3, f.numBatches))])
    finally:
        ctx.set_async_upload(False)
    one_frame(ctx)
    check_against_oracle(decode(ctx), of, colors=False)


# ---- 6. no side effects -------------------------------------------------------------------------------------------------------------
def test_decode_leaves_frames_and_statistics_alone(ctx):
    image, _ = scenes.synth_stream(600_000)
    of = oracle.OracleFile(image.view())
    load(ctx, image.view())
    p = scenes.with_flags(scenes.cameras(160, 90)["overview"], lod_percent=100, cull=1)
    ctx.clear(); ctx.render_hqs_depth(p); ctx.render_hqs_color(p); ctx.resolve_hqs(p)

    def state():
        return ctx.read_framebuffer(full=True), *ctx.read_accum(full=True), ctx.read_rgba(), ctx.stats()

    before = state()
    pts = ctx.decode_points(0, None)
    assert pts.shape == (of.num_batches * PPB, 4)
    after = state()
    for a, b in zip(before[:4], after[:4]):
        assert np.array_equal(a, b)
    assert before[4] == after[4]
    ctx.clear(); ctx.render_basic(p); ctx.resolve_basic(p)
    ofb, ost = of.render_basic(p)
    assert ctx.stats() == ost and np.array_equal(ctx.read_framebuffer(full=True), ofb)
    assert np.array_equal(ctx.read_rgba(), oracle.resolve_basic(p, ofb))


# ---- 7. size --------------------------------------------------------------------------------------------------------------------------
def test_twenty_million_points_in_one_call_into_a_torch_tensor(ctx):
    import torch
    image, st = scenes.synth_stream(20_000_000)
    of = oracle.OracleFile(image.view())
    assert of.num_batches == 306
    f = P.HuffmanFile(image.view())
    ctx.stream_begin(f.header())
    for b0 in range(0, f.numBatches, 100):
        ctx.upload_batches(b0, [f.blob(b) for b in range(b0, min(b0 + 100, f.numBatches))])
    one_frame(ctx)
    pts = ctx.decode_points()
    assert pts.dtype == torch.int32 and pts.is_cuda and tuple(pts.shape) == (306 * PPB, 4)
    host = pts.cpu().numpy()
    for b in range(of.num_batches):
        bad = np.nonzero((host[b * PPB:(b + 1) * PPB, :3] != oracle_xyz(of, b)).any(axis=1))[0]
        assert bad.size == 0, f"batch {b}: {bad.size} points differ from the oracle's, first at {bad[:4]}"
    for b in (0, 305):
        assert np.array_equal(host[b * PPB:(b + 1) * PPB, 3].view(np.uint32), oracle_colors(of, b))
    # HuffmanLasData.points: the same tensor, and world coordinates by torch on the device
    if ctx.layout_name == "point_windows":
        out = torch.empty_like(pts)
        assert torch.equal(ctx.decode_points(0, None, out=out), pts)


def test_resource_points_world_coordinates():
    r = P.Renderer(160, 90)
    try:
        import torch
        image, _ = scenes.synth_stream(600_000)
        las = P.HuffmanLasData.create(image)
        las.load_all(r)
        pts = las.points(r)
        xyz, pts2 = las.points(r, world=True)
        assert torch.equal(pts, pts2) and xyz.dtype == torch.float64 and tuple(xyz.shape) == (pts.shape[0], 3)
        info = las.las_info()
        want = pts[:, :3].cpu().numpy().astype(np.float64) * np.array(info.scale[:]) + np.array(info.offset[:])
        assert np.array_equal(xyz.cpu().numpy(), want)
    finally:
        r.ctx.close()


# ---- 8. the CLI -----------------------------------------------------------------------------------------------------------------------
def run(*cmd):
    res = subprocess.run([str(c) for c in cmd], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    return res


def test_cli_decodes_config1_to_a_las_file(tmp_path):
    build.build_tools()
    image = golden("config1")
    (tmp_path / "config1.huffman").write_bytes(image)
    run(build.DECODE_BIN, tmp_path / "config1.huffman", tmp_path / "config1.las")
    x, y, z, c, las = P.read_las(str(tmp_path / "config1.las"))
    of = oracle.OracleFile(image)
    assert len(x) == of.num_batches * PPB                           # the padded count: the file's header stores no other
    for b in range(of.num_batches):
        s = slice(b * PPB, (b + 1) * PPB)
        assert np.array_equal(np.stack([x[s], y[s], z[s]], axis=1), oracle_xyz(of, b))
        assert np.array_equal(c[s], oracle_colors(of, b))
    g = of.batch(0)
    assert tuple(las.scale) == (g.scale_x, g.scale_y, g.scale_z) and tuple(las.offset) == (g.offset_x, g.offset_y, g.offset_z)


def test_cli_closed_loop_decode_preprocess_decode(tmp_path):
    build.build_tools()
    x, y, z, c = synth_rt()
    image, _ = P.encode_points(x, y, z, c, P.synth_las_info(N_RT), morton_sort=False, pad_tails=True, nthreads=2)
    (tmp_path / "a.huffman").write_bytes(bytes(image.view()))
    run(build.DECODE_BIN, tmp_path / "a.huffman", tmp_path / "a.las")
    run(build.PREPROCESS_BIN, tmp_path / "a.las", tmp_path / "b.huffman", "0", "--pad-tails")
    run(build.DECODE_BIN, tmp_path / "b.huffman", tmp_path / "b.las")
    ax, ay, az, _, _ = P.read_las(str(tmp_path / "a.las"))
    bx, by, bz, _, _ = P.read_las(str(tmp_path / "b.las"))
    assert len(ax) == 327_680 and np.array_equal(ax[:N_RT], x) and np.array_equal(ay[:N_RT], y) and np.array_equal(az[:N_RT], z)
    assert np.array_equal(ax, bx) and np.array_equal(ay, by) and np.array_equal(az, bz)
