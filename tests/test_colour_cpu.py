"""What tests/test_gpu_colour.py rests on, checked without a GPU: the block sets of tests/colour_cases.py cover what they claim (conditions:
a set that misses one fails), the numpy restatement of the BC1 / BC7 decode rule agrees with everything that is not a kernel -- the
oracle, the reference encoders' fixtures, the reference's own BC7 decoder where it is built -- the patched streams parse and decode to
the lattice, the two cameras give the pixel occupancy the GPU tests need, and the oracle's frames over these streams follow from the
restated rule alone. The GPU tests may then compare with the oracle's frames and still rest on the independent decoder."""
import ctypes as C
import os

import numpy as np
import pytest

import pcrhpg24_amd as P
from tests import colour_cases as CC
from tests import oracle, refpin, scenes
from tests.test_bc7 import spec_decode

PPB, BLOCKS = CC.PPB, CC.BLOCKS
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


# ---- coverage -------------------------------------------------------------------------------------------------------------------------
def test_bc1_sets_cover_every_endpoint_pair_selector_and_position():
    """Every (e0, e1, selector) of every channel, every selector at every local position, c0 < c1 and c0 == c1."""
    ex = CC.part("bc1_all", "exhaustive")
    c0, c1, ch, sel = CC.bc1_fields(ex)
    for name, (e0, e1) in ch.items():
        n = 64 if name == "g" else 32
        triple = ((e0 * n + e1)[:, None] * 4 + sel).reshape(-1)
        count = np.bincount(triple, minlength=n * n * 4)
        print(f"BC1 {name}: {np.count_nonzero(count)} of {n * n * 4} (e0, e1, selector) triples")
        assert len(count) == n * n * 4 and count.min() > 0
    at = np.bincount((sel * 16 + np.arange(16)[None, :]).reshape(-1), minlength=64)
    assert at.min() > 0, "a selector never occurs at some local position"
    c0, c1, _, sel = CC.bc1_fields(CC.blocks("bc1_all"))
    less, equal = int((c0 < c1).sum()), int((c0 == c1).sum())
    black = int(((c0 < c1)[:, None] & (sel == 3)).sum())
    print(f"BC1 blocks with c0 < c1: {less}, with c0 == c1: {equal}, of {len(c0)}; pixels a standard decoder makes transparent black: {black}")
    assert less > 0 and equal > 0 and black > 0
    sp = CC.bc1_fields(CC.part("bc1_all", "special"))
    assert (sp[0][:1024] == sp[1][:1024]).all() and (sp[0][1024:2048] < sp[1][1024:2048]).all() and (sp[3][1024:2048] == 3).all()
    combos = {(int(a), int(b), int(CC.selector_word(s[None, :])[0])) for a, b, s in zip(sp[0][2048:2064], sp[1][2048:2064], sp[3][2048:2064])}
    assert combos == {(a, b, w) for a in (0, 0xFFFF) for b in (0, 0xFFFF) for w in (0, 0x55555555, 0xAAAAAAAA, 0xFFFFFFFF)}
    assert np.array_equal(CC.part("bc1_all", "special")[2064:2320], CC.golden_blocks("bc1_ref_blocks.npz"))


def test_bc7_sets_cover_every_endpoint_pair_index_and_mode():
    """Every (E0, E1, index) of every channel at pixels 1 .. 15, where the index is the specification's; all eight upper-bit values
    at pixel 0; blocks that are not mode 6."""
    ex = CC.part("bc7_all", "exhaustive")
    mode, ch, idx = CC.bc7_fields(ex)
    assert (mode == 0x40).all()
    for name in "rgb":
        e0, e1 = ch[name]
        triple = ((e0 * 256 + e1)[:, None] * 16 + idx[:, 1:]).reshape(-1)
        count = np.bincount(triple, minlength=1 << 20)
        print(f"BC7 {name}: {np.count_nonzero(count)} of {1 << 20} (E0, E1, index) triples")
        assert len(count) == 1 << 20 and count.min() > 0
    assert not np.array_equal(ch["r"][0], ch["g"][0]) and not np.array_equal(ch["r"][0], ch["b"][0]) and not np.array_equal(ch["g"][0], ch["b"][0])
    upper = np.bincount(idx[:, 0] >> 1, minlength=8)
    assert len(upper) == 8 and upper.min() > 0
    both = np.bincount((idx[:, 0] >> 1) * 2 + (idx[:, 0] & 1), minlength=16)       # pixel 0's field with either p1
    assert both.min() > 0
    mode_all = CC.bc7_fields(CC.blocks("bc7_all"))[0]
    other = int((mode_all != 0x40).sum())
    print(f"BC7 blocks whose low seven bits are not mode 6: {other} of {len(mode_all)}")
    assert other > 0
    sp = CC.part("bc7_all", "special")
    ref = CC.golden_blocks("bc7_ref_blocks.npz")
    assert np.array_equal(sp[:256], ref)
    for k, (p0, p1) in enumerate((a, b) for a in (0, 1) for b in (0, 1)):
        part = sp[256 * (k + 1):256 * (k + 2)]
        assert np.array_equal(part, CC.with_pbits(ref, p0, p1)) and (part[:, 7] >> 7 == p0).all() and (part[:, 8] & 1 == p1).all()
    assert not sp[1280].any() and (sp[1281] == 255).all()
    frame = CC.blocks("bc7_frame")
    assert np.array_equal(frame[:BLOCKS], sp) and np.array_equal(frame[BLOCKS:2 * BLOCKS], ex[:BLOCKS])
    assert np.array_equal(frame[2 * BLOCKS:3 * BLOCKS], ex[16 * BLOCKS:17 * BLOCKS]) and CC.num_batches("bc7_frame") == 4
    assert CC.num_batches("bc1_all") == 6 and CC.num_batches("bc7_all") == 34


# ---- the restated rule against everything that is not a kernel ----------------------------------------------------------------------
def oracle_pixels(blocks, points, bc7: bool) -> np.ndarray:
    """The oracle's colour of the given point indices over the bytes of `blocks`."""
    flat = np.ascontiguousarray(blocks).reshape(-1)
    fn = oracle.lib().pcr_oracle_decode_bc7 if bc7 else oracle.lib().pcr_oracle_decode_bc1
    ptr = flat.ctypes.data
    return np.fromiter((fn(int(i), ptr) for i in points), np.uint32, len(points))


def test_spec_bc1_is_the_oracles_decode():
    """Every pixel of every BC1 block here (393 216 calls)."""
    b = CC.blocks("bc1_all")
    got = oracle_pixels(b, range(len(b) * 16), False)
    assert np.array_equal(got, CC.spec_bc1(b).reshape(-1))


def test_spec_bc7_is_the_oracles_decode():
    """Every pixel of the special and the random batch; of the exhaustive blocks one pixel each, which walks through the 16 positions
    from block to block and so visits every (E0, E1) pair in either half."""
    for which in ("special", "random"):
        b = CC.part("bc7_all", which)
        assert np.array_equal(oracle_pixels(b, range(len(b) * 16), True), CC.spec_bc7(b).reshape(-1)), which
    ex = CC.part("bc7_all", "exhaustive")
    k = np.arange(len(ex), dtype=np.int64)
    pts = k * 16 + ((k ^ (k >> 4) ^ (k >> 8) ^ (k >> 12) ^ (k >> 16)) & 15)
    assert np.array_equal(oracle_pixels(ex, pts, True), CC.spec_bc7(ex).reshape(-1)[pts])


def test_spec_decoders_reproduce_the_reference_encoders_fixtures():
    """BC1: all 16 pixels of the rgbcx fixture (every block of it has c0 > c1, where the four-colour rule is the standard's too).
    BC7: pixels 1 .. 15 of the bc7enc fixture as its own decoder unpacked them; pixel 0 under the renderers' reading, index << 1 | p1,
    is the specification's pixel wherever that field names the index the specification reads -- and differs somewhere."""
    d = np.load(os.path.join(CC.G, "bc1_ref_blocks.npz"))
    c0, c1, _, _ = CC.bc1_fields(d["blocks"])
    assert (c0 > c1).all()
    assert np.array_equal(CC.spec_bc1(d["blocks"]), d["unpacked"] & 0xFFFFFF)
    d = np.load(os.path.join(CC.G, "bc7_ref_blocks.npz"))
    got = CC.spec_bc7(d["blocks"])
    assert np.array_equal(got[:, 1:], d["unpacked"][:, 1:])
    _, ch, idx = CC.bc7_fields(d["blocks"])
    # pixel 0 by the specification: the 3-bit index at bit 1 of the high quadword
    w = CC.WEIGHTS4[idx[:, 0] >> 1]
    spec0 = sum((((ch[n][0] * (64 - w) + ch[n][1] * w + 32) >> 6) << (8 * k)) for k, n in enumerate("rgba")).astype(np.uint32)
    assert np.array_equal(spec0, d["unpacked"][:, 0])
    for k in range(len(got)):                           # the scalar restatement of tests/test_bc7.py, the renderers' pixel 0 included
        assert np.array_equal(got[k], spec_decode(d["blocks"][k], kernel_quirk=True))
    assert 0 < int((got[:, 0] != d["unpacked"][:, 0]).sum()) < len(got)


def test_spec_bc7_is_the_reference_decoders_unpack_on_mode6_blocks():
    if not refpin.available():
        pytest.skip("oracle/_ref not built (the reference checkout is absent)")
    ref = refpin.ref_lib()
    sp = CC.part("bc7_all", "special")
    mode6 = np.nonzero(CC.bc7_fields(sp)[0] == 0x40)[0]
    assert len(mode6) >= 1280
    want = CC.spec_bc7(sp)
    for k in mode6:
        unp = np.zeros(16, np.uint32)
        blk = np.ascontiguousarray(sp[k])
        assert ref.ref_bc7_unpack(blk.ctypes.data, unp.ctypes.data) == 1
        assert np.array_equal(unp[1:], want[k, 1:]), f"block {k}"


# ---- the streams and the cameras ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=CC.STREAMS)
def loaded(request):
    name = request.param
    return name, oracle.OracleFile(CC.stream(name))


def test_streams_parse_and_decode_to_the_lattice(loaded):
    name, of = loaded
    bc7 = CC.is_bc7(name)
    assert of.num_batches == CC.num_batches(name) and int(of.s.color_format) == (7 if bc7 else 1)
    f = P.HuffmanFile(CC.stream(name))
    assert f.numBatches == of.num_batches
    xyz = CC.points(name)
    for b in range(of.num_batches):
        assert np.array_equal(of.decode_batch(b).reshape(PPB, 3), xyz[b * PPB:(b + 1) * PPB]), f"batch {b}"
    nbytes = of.num_batches * BLOCKS * (16 if bc7 else 8)
    col = np.ctypeslib.as_array(C.cast(of.s.colors, C.POINTER(C.c_uint8)), (nbytes,))
    assert np.array_equal(col, CC.blocks(name).reshape(-1)), "the oracle's colour array is not the constructed blocks"


def traced(name, of, p, variant, npr: int = 64):
    """(pixel, depth bits, record) of every point a frame of camera p draws: npr of every chain, all inside the image, at one depth,
    with the restated rule's colours."""
    assert all(of.batch_lod(b, p, variant)[:2] == (True, npr) for b in range(of.num_batches))
    pix, depth, colour = of.trace_points(p, variant)
    assert len(pix) == of.num_batches * 1024 * npr, "a record falls outside the image"
    assert len(np.unique(depth)) == 1, "the records differ in depth"
    order = CC.walk_order(of.num_batches, npr)
    assert np.array_equal(colour, CC.spec_colours(name)[order]), "the trace's colours are not the restated rule's"
    return pix, depth, order


def test_one_per_pixel_gives_every_record_a_pixel_of_its_own(loaded):
    name, of = loaded
    p = CC.one_per_pixel(name)
    for variant in (oracle.MEM_ITER, oracle.HQS):
        pix, _, _ = traced(name, of, p, variant)
        shared = len(pix) - len(np.unique(pix))
        print(f"{name} one_per_pixel {p.width} x {p.height}: {len(pix)} records, {shared} without a pixel of their own")
        assert shared == 0


def test_many_per_pixel_gives_every_drawn_pixel_sixteen_records_or_more(loaded):
    name, of = loaded
    p = CC.many_per_pixel(name)
    for variant in (oracle.MEM_ITER, oracle.HQS):
        pix, _, _ = traced(name, of, p, variant)
        count = np.bincount(pix, minlength=p.width * p.height)
        drawn = count[count > 0]
        print(f"{name} many_per_pixel {p.width} x {p.height}: {len(drawn)} pixels drawn, {drawn.min()} .. {drawn.max()} records each, mean {drawn.mean():.1f}")
        assert drawn.min() >= 16


# ---- the oracle's frames from the restated rule alone -------------------------------------------------------------------------------
# (camera, lod_percent, the points of a chain the frame draws): the projected size of a batch decides, lod_percent is only its floor --
# under one_per_pixel a batch is hundreds of pixels wide and every chain is drawn whole whatever the floor
FRAMES = [("one_per_pixel", 100, 64), ("one_per_pixel", 50, 64), ("one_per_pixel", 10, 64),
          ("many_per_pixel", 100, 64), ("many_per_pixel", 50, 32), ("many_per_pixel", 10, 19)]


def frame_camera(name, camera, lod):
    return scenes.with_flags(getattr(CC, camera)(name), lod_percent=lod)


@pytest.mark.parametrize("camera,lod,npr", FRAMES)
def test_oracle_basic_frame_is_the_minimum_of_the_spec_colours(camera, lod, npr):
    """Basic, BC1: all depths are equal, so a pixel's word is depth << 32 | the smallest colour among its records (one_per_pixel:
    the colour of its only record)."""
    name = "bc1_all"
    of = oracle.OracleFile(CC.stream(name))
    p = frame_camera(name, camera, lod)
    pix, depth, order = traced(name, of, p, oracle.MEM_ITER, npr)
    want = of.new_fb(p)
    np.minimum.at(want, pix, (depth.astype(np.uint64) << np.uint64(32)) | CC.spec_colours(name)[order].astype(np.uint64))
    fb, st = of.render_basic(p)
    assert st["points_iterated"] == of.num_batches * 1024 * npr
    assert np.array_equal(fb, want)
    assert int((fb != EMPTY).sum()) == len(np.unique(pix))


@pytest.mark.parametrize("name", ["bc1_all", "bc7_frame"])
@pytest.mark.parametrize("camera,lod,npr", [FRAMES[0], FRAMES[3], FRAMES[5]])
def test_oracle_hqs_sums_are_the_sums_of_the_spec_colours(name, camera, lod, npr):
    """HQS: every record passes the 1 % test (one depth), so RG and BA are the per-pixel sums of the restated rule's r << 32 | g and
    b << 32 | 1 -- the count is the number of records of the pixel."""
    of = oracle.OracleFile(CC.stream(name))
    p = frame_camera(name, camera, lod)
    pix, depth, order = traced(name, of, p, oracle.HQS, npr)
    c = CC.spec_colours(name)[order].astype(np.uint64)
    fb, _ = of.render_hqs_depth(p)
    want_fb = of.new_fb(p)
    want_fb[np.unique(pix)] = np.uint64(int(depth[0]) << 32)
    assert np.array_equal(fb, want_fb)
    rg, ba, _ = of.render_hqs_color(p, fb)
    want_rg, want_ba = np.zeros_like(rg), np.zeros_like(ba)
    np.add.at(want_rg, pix, ((c & np.uint64(255)) << np.uint64(32)) | ((c >> np.uint64(8)) & np.uint64(255)))
    np.add.at(want_ba, pix, (((c >> np.uint64(16)) & np.uint64(255)) << np.uint64(32)) | np.uint64(1))
    assert np.array_equal(rg, want_rg) and np.array_equal(ba, want_ba)
    assert np.array_equal(ba & np.uint64(0xFFFFFFFF), np.bincount(pix, minlength=len(ba)).astype(np.uint64))
