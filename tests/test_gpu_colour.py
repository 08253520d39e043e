"""Every kernel that decodes a colour block -- k_decode_points, decode_chain() behind the selections, k_grid, k_render in the basic and
the HQS colour pass, k_pick / k_pick_fetch -- on the constructed BC1 / BC7 blocks of tests/colour_cases.py: every endpoint pair with
every selector or index, c0 <= c1, foreign mode bits, the renderers' reading of pixel 0.

Records, selections, grids and picks are compared with the numpy restatement of the decode rule (colour_cases.spec_bc1 / spec_bc7);
frames with the oracle's, which tests/test_colour_cpu.py derives from that restatement alone. Every comparison is byte for byte.
A context per stream and layout is loaded once and shared by the tests of the module."""
import functools

import numpy as np
import pytest

import pcrhpg24_amd as P
from tests import colour_cases as CC
from tests import grid_cases as G
from tests import oracle
from tests import select_cases as S
from tests.test_colour_cpu import FRAMES, frame_camera

pytestmark = pytest.mark.gpu

PPB = CC.PPB
LAYOUTS = {"words": P.Context.LAYOUT_WORDS, "point_windows": P.Context.LAYOUT_POINT_WINDOWS}
WHOLE = ["bc1_all", "bc7_all"]
FRAME_STREAMS = ["bc1_all", "bc7_frame"]
HQS_FRAMES = [FRAMES[0], FRAMES[3], FRAMES[5]]          # one_per_pixel; many_per_pixel whole chains; ... and their first 19 points


@pytest.fixture(scope="module")
def resident():
    """resident(stream, layout): the context that holds the stream in that layout, loaded on first use."""
    made = {}

    def get(name, layout):
        if (name, layout) not in made:
            c = P.Context(0)
            made[name, layout] = c
            c.set_stream_layout(LAYOUTS[layout])
            f = P.HuffmanFile(CC.stream(name))
            c.stream_begin(f.header())
            for b in range(f.numBatches):
                c.upload_batch(b, f.blob(b))
            assert c.stream_color_format() == (7 if CC.is_bc7(name) else 1)
        return made[name, layout]

    yield get
    for c in made.values():
        c.close()


@pytest.fixture(params=list(LAYOUTS))
def layout(request):
    return request.param


@functools.lru_cache(maxsize=None)
def records(name: str) -> np.ndarray:
    """What read_points has to return: the lattice with the restated rule's colours (the record has no room for BC7's alpha)."""
    out = np.empty(len(CC.points(name)), P.POINT_DTYPE)
    xyz = CC.points(name)
    out["x"], out["y"], out["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    out["color"] = CC.spec_colours(name) & np.uint32(0xFFFFFF)
    out.setflags(write=False)
    return out


def same_records(got, want, what):
    assert got.dtype == want.dtype and len(got) == len(want), f"{what}: {len(got)} records, {len(want)} expected"
    if got.tobytes() != want.tobytes():
        bad = np.nonzero(got != want)[0]
        xyz = sum(int((got[k][bad] != want[k][bad]).sum()) for k in "xyz")
        raise AssertionError(f"{what}: {bad.size} records differ ({xyz} coordinates), first at {bad[:4]}: "
                             f"colours {[hex(v) for v in got['color'][bad[:4]]]}, expected {[hex(v) for v in want['color'][bad[:4]]]}")


def from_tensor(t) -> np.ndarray:
    return np.ascontiguousarray(t.cpu().numpy()).view(P.POINT_DTYPE).reshape(-1)


# ---- k_decode_points ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WHOLE)
def test_read_points_are_the_lattice_with_the_spec_colours(resident, layout, name):
    c = resident(name, layout)
    same_records(c.read_points(), records(name), "read_points")
    if layout == "point_windows":
        same_records(from_tensor(c.decode_points()), records(name), "decode_points")


# ---- decode_chain ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WHOLE)
def test_select_box_cuts_a_lattice_row_off_every_batch(resident, layout, name):
    """A box cannot cut through every tile of a square layout at once: one call per tile row (its batches are consecutive), with a
    box that begins at the row's second lattice row. Every batch of the call straddles it, so its records come from decode_chain."""
    c = resident(name, layout)
    cols, rows = CC.tiles(name)
    want_all = records(name)
    for ty in range(rows):
        first = ty * cols
        count = min(cols, CC.num_batches(name) - first)
        box = ((S.INT32_MIN, (ty * CC.SIDE + 1) * CC.STEP, S.INT32_MIN), (S.INT32_MAX,) * 3)
        got = from_tensor(c.select_box(box, first, count))
        st = dict(c.select_stats)
        ref = want_all[first * PPB:(first + count) * PPB]
        want = ref[S.in_box(np.stack([ref["x"], ref["y"], ref["z"]], axis=1), box)]
        assert len(want) == count * (PPB - CC.SIDE)
        assert st == {"batches_outside": 0, "batches_inside": 0, "batches_straddling": count, "points_selected": len(want)}, f"tile row {ty}"
        same_records(got, want, f"select_box, tile row {ty}")


@pytest.mark.parametrize("name", WHOLE)
def test_select_box_that_holds_everything(resident, layout, name):
    c = resident(name, layout)
    got = from_tensor(c.select_box(S.FULL))
    n = CC.num_batches(name)
    assert c.select_stats == {"batches_outside": 0, "batches_inside": n, "batches_straddling": 0, "points_selected": n * PPB}
    same_records(got, records(name), "select_box")


# ---- k_grid ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell,windowed", [(1000, False), (4000, True)], ids=["cell1000-direct", "cell4000-windowed"])
@pytest.mark.parametrize("name", WHOLE)
def test_read_grid_planes(resident, layout, name, cell, windowed):
    """One record per cell (a batch covers 65 536 cells: no LDS window), and 16 records per cell (4096 cells a batch: windowed);
    top = max and bottom = min of (z ^ 0x80000000) << 32 | colour over the restated rule's records."""
    c = resident(name, layout)
    cols, rows = CC.tiles(name)
    per_tile = CC.SIDE * CC.STEP // cell
    grid = (0, 0, cell, cols * per_tile, rows * per_tile)
    top, bottom, count = c.read_grid(grid)
    n = CC.num_batches(name)
    assert c.grid_stats == {"batches_outside": 0, "batches_windowed": n if windowed else 0, "batches_direct": 0 if windowed else n}
    want = G.reference(records(name), grid)
    for got, ref, what in zip((top, bottom, count), want, ("top", "bottom", "count")):
        assert got.dtype == ref.dtype and got.shape == ref.shape
        assert got.tobytes() == ref.tobytes(), f"{what}: {(got != ref).sum()} of {got.size} cells differ, first at {np.argwhere(got != ref)[:4].tolist()}"
    filled = count[count > 0]
    assert filled.min() == filled.max() == (cell // CC.STEP) ** 2


# ---- k_render -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_file(name):
    return oracle.OracleFile(CC.stream(name))


@functools.lru_cache(maxsize=None)
def oracle_basic(name, camera, lod):
    p = frame_camera(name, camera, lod)
    fb, st = oracle_file(name).render_basic(p)
    return p, fb, st, oracle.resolve_basic(p, fb)


@functools.lru_cache(maxsize=None)
def oracle_hqs(name, camera, lod):
    p = frame_camera(name, camera, lod)
    of = oracle_file(name)
    fb, st = of.render_hqs_depth(p)
    rg, ba, _ = of.render_hqs_color(p, fb)
    return p, fb, st, rg, ba, oracle.resolve_hqs(p, fb, rg, ba)


def same_words(got, want, what):
    assert got.shape == want.shape
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} words differ, first at {bad[:4]}: {[hex(v) for v in got[bad[:4]]]}, expected {[hex(v) for v in want[bad[:4]]]}"


@pytest.mark.parametrize("camera,lod,npr", FRAMES, ids=[f"{c}-lod{l}" for c, l, _ in FRAMES])
def test_basic_frames_of_the_bc1_stream(resident, layout, camera, lod, npr):
    """Both places where k_render puts a BC1 colour into a framebuffer word: the point loop (every point but a segment's last) and the
    scatter behind a segment -- which a chain cut at npr = 32 or 19 reaches with other pixels of a block than its last."""
    c = resident("bc1_all", layout)
    p, ofb, ost, oimg = oracle_basic("bc1_all", camera, lod)
    assert ost["points_iterated"] == CC.num_batches("bc1_all") * 1024 * npr
    c.set_image_size(p.width, p.height)
    c.clear(); c.render_basic(p); c.resolve_basic(p)
    assert c.stats() == ost
    same_words(c.read_framebuffer(full=True), ofb, "basic")
    same_words(c.read_rgba(), oimg, "resolve_basic")


@pytest.mark.parametrize("camera,lod,npr", HQS_FRAMES, ids=[f"{c}-lod{l}" for c, l, _ in HQS_FRAMES])
@pytest.mark.parametrize("name", FRAME_STREAMS)
def test_hqs_frames(resident, layout, name, camera, lod, npr):
    """Depth, colour sums and resolve. many_per_pixel: a chain's consecutive records share a pixel, so the colour pass sums runs of
    arbitrary colours in its 16-bit register halves."""
    c = resident(name, layout)
    p, ofb, ost, org, oba, oimg = oracle_hqs(name, camera, lod)
    assert ost["points_iterated"] == CC.num_batches(name) * 1024 * npr
    c.set_image_size(p.width, p.height)
    c.clear(); c.render_hqs_depth(p)
    assert c.stats() == ost
    same_words(c.read_framebuffer(full=True), ofb, "HQS depth")
    c.render_hqs_color(p); c.resolve_hqs(p)
    rg, ba = c.read_accum(full=True)
    same_words(rg, org, "RG sums")
    same_words(ba, oba, "BA sums")
    same_words(c.read_rgba(), oimg, "resolve_hqs")


def test_basic_method_refuses_the_bc7_stream(resident, layout):
    c = resident("bc7_frame", layout)
    p = CC.many_per_pixel("bc7_frame")
    c.set_image_size(p.width, p.height)
    with pytest.raises(P.PcrError, match="BC7"):
        c.render_basic(p)


# ---- k_pick / k_pick_fetch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FRAME_STREAMS)
def test_pick_returns_the_pixels_record_with_the_spec_colour(resident, layout, name):
    c = resident(name, layout)
    p = CC.one_per_pixel(name)
    c.set_image_size(p.width, p.height)
    pix, depth, _ = oracle_file(name).trace_points(p)
    order = CC.walk_order(CC.num_batches(name))
    assert len(pix) == len(order) == len(np.unique(pix))
    want = records(name)
    for k in np.random.default_rng(16).choice(len(pix), 16, replace=False):
        got = c.pick(p, int(pix[k] % p.width), int(pix[k] // p.width), 0)
        assert got is not None, f"pixel {pix[k]} holds record {order[k]}"
        pt, hit = got
        assert (hit.pixel, hit.depth_bits, hit.index) == (pix[k], depth[k], order[k])
        assert bytes(pt) == want[order[k]].tobytes(), f"record {order[k]}: colour {pt.color:#x}, expected {want['color'][order[k]]:#x}"
