"""pcr_grid_clear / pcr_grid_accumulate / pcr_grid_unpack / pcr_read_grid: a loaded stream rasterized top-down on the GPU.

The contract is one sentence -- every cell holds the max / min / count over exactly the records pcr_decode_points writes that
fall into it -- and max, min and add do not depend on the order, so every comparison here is tobytes() equality with
np.maximum.at / np.minimum.at / np.bincount over Context.read_points of the same range (tests/grid_cases.py), no tolerances.
Every case runs for a context loaded with PCR_LAYOUT_WORDS, PCR_LAYOUT_POINT_WINDOWS and PCR_LAYOUT_BOTH (there through both
variants, which have to agree), as tests/test_gpu_select.py does. tests/test_grid_cpu.py checks on the CPU that the grids of
tests/grid_cases.py put the batches into the classes claimed."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import _native as N
from pcrhpg24_amd import build
from tests import grid_cases as G
from tests import oracle, scenes
from tests import select_cases as S

pytestmark = pytest.mark.gpu

PPB = S.PPB
PCR_E_ARG = -1
LAYOUTS = {"words": P.Context.LAYOUT_WORDS, "point_windows": P.Context.LAYOUT_POINT_WINDOWS, "both": P.Context.LAYOUT_BOTH}
PLANES = ("top", "bottom", "counts")
SENT64, SENT32 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A
SYNTH_GRID = G.CASES[1][1]                                                  # synth, all three classes


@pytest.fixture(params=list(LAYOUTS))
def ctx(request):
    c = P.Context(0)
    c.set_stream_layout(LAYOUTS[request.param])
    c.set_image_size(160, 90)
    c.layout_name = request.param
    yield c
    c.close()


def one_frame(c):
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
        one_frame(c)
    return f


def variants(c):
    return (P.Context.VARIANT_AUTO,) if c.layout_name != "both" else (P.Context.VARIANT_WORDS, P.Context.VARIANT_POINT_WINDOWS)


def through_variants(c, fn):
    """fn() under every decode variant the context's layout holds; the results (tuples of numpy arrays) have to agree."""
    outs = []
    for v in variants(c):
        c.set_render_variant(v)
        outs.append(fn())
    c.set_render_variant(P.Context.VARIANT_AUTO)
    for o in outs[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(o, outs[0])), "the two layouts of one stream give different results"
    return outs[0]


def stats_array(c):
    return np.array([c.grid_stats[k] for k in ("batches_outside", "batches_windowed", "batches_direct")])


def stats_dict(a):
    return dict(zip(("batches_outside", "batches_windowed", "batches_direct"), (int(v) for v in a)))


def read_grid(c, grid, clip=None, first=0, count=None, flags=0):
    """Context.read_grid under every variant: (top, bottom, count), and the classes it reported."""
    def go():
        return *c.read_grid(grid, clip, first, count, flags), stats_array(c)
    *planes, st = through_variants(c, go)
    return tuple(planes), stats_dict(st)


def new_planes(c, grid, which=PLANES, clear=True):
    """Torch planes for the grid, the ones named in `which` (the others None), cleared by grid_clear."""
    import torch
    dev = f"cuda:{c.device}"
    shape = (grid[4], grid[3])
    t = {k: None for k in PLANES}
    for k in which:
        t[k] = torch.full(shape, SENT64 if k != "counts" else SENT32, dtype=torch.int64 if k != "counts" else torch.int32, device=dev)
    if clear:
        c.grid_clear(grid, **t)
    return t


def host(t):
    """numpy (uint64, uint64, uint32) of a dict of torch planes; None stays None."""
    return tuple(None if t[k] is None else t[k].cpu().numpy().view(np.uint64 if k != "counts" else np.uint32) for k in PLANES)


def torch_grid(c, grid, which=PLANES, clip=None, first=0, count=None, flags=0):
    """grid_clear + grid_accumulate on torch planes under every variant: the planes asked for and the classes."""
    def go():
        t = new_planes(c, grid, which)
        c.grid_accumulate(grid, clip=clip, first=first, count=count, flags=flags, **t)
        return *(p for p in host(t) if p is not None), stats_array(c)
    *planes, st = through_variants(c, go)
    return dict(zip(which, planes)), stats_dict(st)


def same(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert got.tobytes() == want.tobytes(), f"{what}: {(got != want).sum()} of {got.size} cells differ, first at {np.argwhere(got != want)[:4].tolist()}"


def check_grid(c, grid, ref, bounds=None, clip=None, first=0, count=None):
    """read_grid, the torch path with all planes and with every plane alone, and all of it again with PCR_GRID_NO_WINDOW, equal
    the numpy reference over `ref` (read_points of the same range); with `bounds` the reported classes equal the classifier's."""
    want = dict(zip(PLANES, G.reference(ref, grid, clip)))
    plain = None                                                            # the classes without PCR_GRID_NO_WINDOW
    for flags in (0, G.NO_WINDOW):
        cls = None if bounds is None else G.class_counts(G.classify(bounds, grid, clip, flags))
        got, st = read_grid(c, grid, clip, first, count, flags)
        for k, g in zip(PLANES, got):
            same(g, want[k], f"read_grid {k} flags {flags}")
        runs = [st]
        for which in (PLANES, ("top",), ("bottom",), ("counts",)):
            got, st = torch_grid(c, grid, which, clip, first, count, flags)
            for k in which:
                same(got[k], want[k], f"planes {which}: {k} flags {flags}")
            runs.append(st)
        for st in runs:
            assert sum(st.values()) == len(ref) // PPB
            assert cls is None or st == cls, (st, cls)
            assert not flags or st["batches_windowed"] == 0
        plain = plain or runs[0]
    return want, plain


# ---- 1. every case against the reference --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(G.CASES)), ids=[f"{c[0]}-{c[1][2] if c[1] else 'own'}x{c[1][3] if c[1] else ''}" for c in G.CASES])
@pytest.mark.parametrize("frame", [True, False], ids=["after_frame", "before_any_frame"])
def test_grid_equals_numpy_over_read_points(ctx, case, frame):
    name, grid, classes = G.CASES[case]
    image = G.stream(name)
    of = oracle.OracleFile(image)
    load(ctx, image, frame=frame)
    bounds = S.oracle_bounds(of)
    grid = G.grid_over(bounds) if grid is None else grid
    ref = through_variants(ctx, lambda: (ctx.read_points(),))[0]
    assert len(ref) == of.num_batches * PPB
    want, st = check_grid(ctx, grid, ref, bounds)
    print(f"{name} {grid}: {int(want['counts'].sum())} of {len(ref)} records in {int((want['counts'] > 0).sum())} of {want['counts'].size} cells, {st}")
    assert want["counts"].sum() > 0
    if classes is not None:
        assert st == G.class_counts(classes)
    if name == "plateau":
        # the case the tie rule decides: a cell whose top z is held by records of different colours
        m, idx = G.cells_of(ref, grid)
        z, col = ref["z"][m].astype(np.int64), ref["color"][m].astype(np.int64)
        topz = G.unpack(want["top"], G.EMPTY_TOP)[0].ravel().astype(np.int64)
        holders = z == topz[idx]
        lo, hi = np.full(topz.size, 1 << 40, np.int64), np.full(topz.size, -1, np.int64)
        np.minimum.at(lo, idx[holders], col[holders]); np.maximum.at(hi, idx[holders], col[holders])
        assert (hi > lo).sum() >= 1, "no cell's top z is held by records of different colours"
        print(f"plateau: {(hi > lo).sum()} cells decided by the tie rule")
    # a 1-cell grid around known points (a padding duplicate or a chain start may put more than one record there)
    for k in (0, len(ref) // 2 + 777, len(ref) - 1):
        one = (int(ref["x"][k]), int(ref["y"][k]), 1, 1, 1)
        w1, _ = check_grid(ctx, one, ref, bounds)
        assert w1["counts"][0, 0] >= 1


# ---- 2. clip ---------------------------------------------------------------------------------------------------------------------
def test_clip(ctx):
    image = G.stream("synth")
    of = oracle.OracleFile(image)
    load(ctx, image)
    bounds = S.oracle_bounds(of)
    ref = ctx.read_points()
    grid = G.CASES[0][1]
    slab = ((S.INT32_MIN, S.INT32_MIN, 30000), (S.INT32_MAX, S.INT32_MAX, 40000))
    want, _ = check_grid(ctx, grid, ref, bounds, clip=slab)
    full = G.reference(ref, grid)
    assert 0 < want["counts"].sum() < full[2].sum() and not np.array_equal(want["top"], full[0])
    # a clip that cuts x and y as well, with edges inside cells
    check_grid(ctx, SYNTH_GRID, ref, bounds, clip=((600_123, 610_456, 20_000), (900_001, 777_777, 60_000)))
    for clip in (S.EMPTY, S.NOTHING):
        for flags in (0, G.NO_WINDOW):
            got, st = read_grid(ctx, grid, clip, flags=flags)
            assert st == {"batches_outside": of.num_batches, "batches_windowed": 0, "batches_direct": 0}
            assert (got[0] == G.EMPTY_TOP).all() and (got[1] == G.EMPTY_BOTTOM).all() and (got[2] == 0).all()
            got, st = torch_grid(ctx, grid, clip=clip, flags=flags)
            assert st["batches_outside"] == of.num_batches
            assert (got["top"] == G.EMPTY_TOP).all() and (got["bottom"] == G.EMPTY_BOTTOM).all() and (got["counts"] == 0).all()


# ---- 3. accumulate ---------------------------------------------------------------------------------------------------------------
def test_sub_ranges_accumulate_to_the_whole_range(ctx):
    image = G.stream("synth")
    of = oracle.OracleFile(image)
    load(ctx, image)
    nb = of.num_batches
    bounds = S.oracle_bounds(of)
    ref = ctx.read_points()
    grid = SYNTH_GRID
    want = G.reference(ref, grid)
    for v in variants(ctx):
        ctx.set_render_variant(v)
        t = new_planes(ctx, grid)
        total = np.zeros(3, np.int64)
        for first, count in ((0, 3), (3, 1), (4, 0), (4, 5), (9, None)):
            st = ctx.grid_accumulate(grid, first=first, count=count, **t)
            end = nb if count is None else first + count
            assert st == G.class_counts(G.classify(bounds[first:end], grid))
            total += stats_array(ctx)
        for g, w, k in zip(host(t), want, PLANES):
            same(g, w, f"accumulated {k}")
        assert stats_dict(total) == G.class_counts(G.classify(bounds, grid))
        # a second pass over the whole range: the counts double, max and min stay
        ctx.grid_accumulate(grid, **t)
        got = host(t)
        same(got[0], want[0], "top after a second pass"); same(got[1], want[1], "bottom after a second pass")
        same(got[2], want[2] * np.uint32(2), "counts after a second pass")
    ctx.set_render_variant(P.Context.VARIANT_AUTO)
    # sub-ranges on their own against the reference of their records
    for first, count in ((0, 3), (3, 1), (4, 0), (9, None), (nb, None)):
        end = nb if count is None else first + count
        got, st = read_grid(ctx, grid, None, first, count)
        for g, w, k in zip(got, G.reference(ref[first * PPB:end * PPB], grid), PLANES):
            same(g, w, f"range {first}+{count} {k}")
        assert sum(st.values()) == end - first


def test_two_shards_accumulate_to_the_single_contexts_planes(ctx):
    image = G.stream("synth")
    f = load(ctx, image)
    grid = SYNTH_GRID
    whole, _ = read_grid(ctx, grid)
    half = f.numBatches // 2
    other = P.Context(0)
    try:
        other.set_stream_layout(LAYOUTS[ctx.layout_name]); other.set_image_size(160, 90); other.layout_name = ctx.layout_name
        load(ctx, image, first=0, count=half)
        load(other, image, first=half, count=f.numBatches - half)
        t = new_planes(ctx, grid)
        a = ctx.grid_accumulate(grid, **t)
        b = other.grid_accumulate(grid, **t)
        for g, w, k in zip(host(t), whole, PLANES):
            same(g, w, f"two shards {k}")
        assert sum(a.values()) == half and sum(b.values()) == f.numBatches - half and whole[2].sum() > 0
    finally:
        other.close()


# ---- 4. unpack, read_grid against the torch path ------------------------------------------------------------------------------------
def test_unpack_and_read_grid_against_the_torch_path(ctx):
    import torch
    image = G.stream("escape_heavy")                                        # negative z: the bias
    load(ctx, image)
    grid = G.CASES[5][1]
    (top, bottom, count), _ = read_grid(ctx, grid)
    got, _ = torch_grid(ctx, grid)
    same(got["top"], top, "top"); same(got["bottom"], bottom, "bottom"); same(got["counts"], count, "counts")
    assert (count == 0).any() and (count > 0).any(), "the grid needs empty and filled cells"
    dev = f"cuda:{ctx.device}"
    for words, which, empty in ((top, P.GRID_TOP, G.EMPTY_TOP), (bottom, P.GRID_BOTTOM, G.EMPTY_BOTTOM)):
        t = torch.from_numpy(words.view(np.int64)).to(dev)
        h, rgba = ctx.grid_unpack(grid, t, which)
        wh, wr = G.unpack(words, empty)
        assert h.dtype == torch.int32 and tuple(h.shape) == (grid[4], grid[3]) == tuple(rgba.shape)
        same(h.cpu().numpy(), wh, "height"); same(rgba.cpu().numpy().view(np.uint32), wr, "rgba")
        assert (wh[count == 0] == S.INT32_MIN).all() and (wr[count == 0] == 0).all() and (wh[count > 0] != S.INT32_MIN).all()
        # either output alone
        sent = torch.full((grid[4], grid[3]), SENT32, dtype=torch.int32, device=dev)
        g = N.Grid(*grid, 0)
        assert ctx.lib.pcr_grid_unpack(ctx.h, C.byref(g), C.c_void_p(t.data_ptr()), which, C.c_void_p(sent.data_ptr()), None) == 0
        ctx.synchronize()
        same(sent.cpu().numpy(), wh, "height alone")
        assert ctx.lib.pcr_grid_unpack(ctx.h, C.byref(g), C.c_void_p(t.data_ptr()), which, None, C.c_void_p(sent.data_ptr())) == 0
        ctx.synchronize()
        same(sent.cpu().numpy().view(np.uint32), wr, "rgba alone")
    assert (G.unpack(top, G.EMPTY_TOP)[0] < 0).any()


# ---- 5. errors ---------------------------------------------------------------------------------------------------------------------
def test_errors_are_pcr_e_arg_with_a_message_and_write_nothing(ctx):
    import torch
    lib, h = ctx.lib, ctx.h
    dev = f"cuda:{ctx.device}"
    grid = SYNTH_GRID
    cells = grid[3] * grid[4]
    top = torch.full((cells + 1,), SENT64, dtype=torch.int64, device=dev)
    bottom, cnt = top.clone(), torch.full((cells + 1,), SENT32, dtype=torch.int32, device=dev)
    out_h, out_c = cnt.clone(), cnt.clone()
    hosts = [np.full(cells, SENT64, np.uint64), np.full(cells, SENT64, np.uint64), np.full(cells, SENT32, np.uint32)]
    st = N.GridStats(7, 7, 7)
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)

    def refused(rc):
        assert rc == PCR_E_ARG
        assert (lib.pcr_last_error(h) or b"") != b""

    def accumulate(first=0, count=-1, g=grid, pg=True, t=None, b=None, c=None, flags=0):
        gg = N.Grid(*g)
        return lib.pcr_grid_accumulate(h, first, count, C.byref(gg) if pg else None, None, t or ptr(top), b or ptr(bottom), c or ptr(cnt), flags, C.byref(st))

    def read(first=0, count=-1, g=grid, pg=True, flags=0):
        gg = N.Grid(*g)
        return lib.pcr_read_grid(h, first, count, C.byref(gg) if pg else None, None, *(a.ctypes.data for a in hosts), flags, C.byref(st))

    refused(accumulate()); refused(read())                                  # no stream loaded
    load(ctx, G.stream("synth"))
    nb = ctx.batches_loaded
    ox, oy, cell, w, hh = grid
    bad_grids = [(ox, oy, 0, w, hh), (ox, oy, -5, w, hh), (ox, oy, cell, 0, hh), (ox, oy, cell, w, -1), (ox, oy, cell, 8193, 8192),
                 (ox, oy, cell, S.INT32_MAX, S.INT32_MAX), (ox, oy, cell, w, hh, 1)]
    for call in (accumulate, read):
        refused(call(nb - 1, 2)); refused(call(-1, 1)); refused(call(nb + 1, -1))      # a range outside the resident batches
        refused(call(pg=False))                                             # a NULL grid
        for g in bad_grids:
            refused(call(g=g))
        refused(call(flags=2)); refused(call(flags=0x80000001))             # unknown flag bits
    refused(accumulate(t=ptr(top, 4))); refused(accumulate(b=ptr(bottom, 4))); refused(accumulate(c=ptr(cnt, 2)))       # misaligned
    for g in bad_grids:
        gg = N.Grid(*g)
        refused(lib.pcr_grid_clear(h, C.byref(gg), ptr(top), ptr(bottom), ptr(cnt)))
        refused(lib.pcr_grid_unpack(h, C.byref(gg), ptr(top), P.GRID_TOP, ptr(out_h), ptr(out_c)))
    gg = N.Grid(*grid)
    refused(lib.pcr_grid_clear(h, None, ptr(top), ptr(bottom), ptr(cnt)))
    refused(lib.pcr_grid_clear(h, C.byref(gg), ptr(top, 4), None, None)); refused(lib.pcr_grid_clear(h, C.byref(gg), None, None, ptr(cnt, 2)))
    refused(lib.pcr_grid_unpack(h, None, ptr(top), P.GRID_TOP, ptr(out_h), ptr(out_c)))
    refused(lib.pcr_grid_unpack(h, C.byref(gg), None, P.GRID_TOP, ptr(out_h), ptr(out_c)))
    refused(lib.pcr_grid_unpack(h, C.byref(gg), ptr(top), 2, ptr(out_h), ptr(out_c)))
    refused(lib.pcr_grid_unpack(h, C.byref(gg), ptr(top, 4), P.GRID_TOP, ptr(out_h), ptr(out_c)))
    refused(lib.pcr_grid_unpack(h, C.byref(gg), ptr(top), P.GRID_TOP, ptr(out_h, 2), ptr(out_c)))
    ctx.synchronize(); torch.cuda.synchronize()
    for t, s in ((top, SENT64), (bottom, SENT64), (cnt, SENT32), (out_h, SENT32), (out_c, SENT32)):
        assert (t == s).all().item(), "a refused call wrote into a buffer"
    assert (hosts[0] == SENT64).all() and (hosts[1] == SENT64).all() and (hosts[2] == SENT32).all()
    assert (st.batches_outside, st.batches_windowed, st.batches_direct) == (7, 7, 7)
    # what is not an error: all planes NULL (no work), 0 batches, a NULL stats, the largest grid there is
    assert lib.pcr_grid_accumulate(h, 0, -1, C.byref(gg), None, None, None, None, 0, C.byref(st)) == 0
    assert (st.batches_outside, st.batches_windowed, st.batches_direct) == (0, 0, 0)
    assert lib.pcr_grid_accumulate(h, nb, -1, C.byref(gg), None, ptr(top), ptr(bottom), ptr(cnt), 0, C.byref(st)) == 0 and st.batches_outside == 0
    assert lib.pcr_grid_accumulate(h, 2, 0, C.byref(gg), None, ptr(top), ptr(bottom), ptr(cnt), 0, None) == 0
    assert lib.pcr_grid_clear(h, C.byref(gg), None, None, None) == 0
    ctx.synchronize()
    assert (top == SENT64).all().item() and (cnt == SENT32).all().item()
    # a refused call leaves the context usable; the planes end where the grid ends
    ref = ctx.read_points()
    check_grid(ctx, grid, ref)
    assert lib.pcr_grid_clear(h, C.byref(gg), ptr(top), ptr(bottom), ptr(cnt)) == 0
    assert lib.pcr_grid_accumulate(h, 0, -1, C.byref(gg), None, ptr(top), ptr(bottom), ptr(cnt), 0, None) == 0
    ctx.synchronize()
    want = G.reference(ref, grid)
    same(top[:cells].cpu().numpy().view(np.uint64), want[0].ravel(), "top"); same(cnt[:cells].cpu().numpy().view(np.uint32), want[2].ravel(), "counts")
    assert top[cells].item() == SENT64 and bottom[cells].item() == SENT64 and cnt[cells].item() == SENT32


# ---- 6. no side effects ------------------------------------------------------------------------------------------------------------
def test_grid_leaves_frames_and_statistics_alone(ctx):
    image = G.stream("synth")
    of = oracle.OracleFile(image)
    load(ctx, image)
    p = scenes.with_flags(scenes.cameras(160, 90)["overview"], lod_percent=100, cull=1)
    ctx.clear(); ctx.render_hqs_depth(p); ctx.render_hqs_color(p); ctx.resolve_hqs(p)

    def state():
        return ctx.read_framebuffer(full=True), *ctx.read_accum(full=True), ctx.read_rgba(), ctx.stats()

    before = state()
    top, bottom, count = ctx.read_grid(SYNTH_GRID)
    assert count.sum() > 0 and min(ctx.grid_stats.values()) >= 1
    got, _ = torch_grid(ctx, G.CASES[0][1], flags=G.NO_WINDOW)
    assert got["counts"].sum() > 0
    after = state()
    for a, b in zip(before[:4], after[:4]):
        assert np.array_equal(a, b)
    assert before[4] == after[4]
    ctx.clear(); ctx.render_basic(p); ctx.resolve_basic(p)
    ofb, ost = of.render_basic(p)
    assert ctx.stats() == ost and np.array_equal(ctx.read_framebuffer(full=True), ofb)
    assert np.array_equal(ctx.read_rgba(), oracle.resolve_basic(p, ofb))


# ---- 7. size ---------------------------------------------------------------------------------------------------------------------------
def test_twenty_million_points(ctx):
    import torch
    image, _ = scenes.synth_stream(20_000_000)
    f = P.HuffmanFile(image.view())
    assert f.numBatches == 306
    ctx.stream_begin(f.header())
    for b0 in range(0, f.numBatches, 100):
        ctx.upload_batches(b0, [f.blob(b) for b in range(b0, min(b0 + 100, f.numBatches))])
    one_frame(ctx)
    ref = ctx.decode_points()                                               # (tests/test_gpu_decode.py holds it against the oracle)
    per_batch = ref.view(306, PPB, 4)[:, :, :3]
    bounds = torch.cat([per_batch.amin(dim=1), per_batch.amax(dim=1)], dim=1).cpu().numpy()
    x, y, z = (ref[:, k].to(torch.int64) for k in range(3))
    key = (z << 32) | (ref[:, 3].to(torch.int64) & 0xFFFFFFFF)             # signed order of this = unsigned order of K = key ^ 1 << 63
    sign = torch.tensor(-(1 << 63), dtype=torch.int64, device=ref.device)
    # cell 4000: every batch windowed or direct by its box; cell 100: the largest grid there is (2^26 cells), all direct
    for grid in ((0, 0, 4000, 250, 250), (0, 0, 100, 8192, 8192)):
        ox, oy, cell, w, h = grid
        cx, cy = (x - ox) // cell, (y - oy) // cell
        m = (x >= ox) & (y >= oy) & (cx < w) & (cy < h)
        idx = (cx + cy * w)[m]
        want_top = torch.full((w * h,), -(1 << 63), dtype=torch.int64, device=ref.device).scatter_reduce(0, idx, key[m], "amax") ^ sign
        want_bottom = torch.full((w * h,), (1 << 63) - 1, dtype=torch.int64, device=ref.device).scatter_reduce(0, idx, key[m], "amin") ^ sign
        want_count = torch.bincount(idx, minlength=w * h).to(torch.int32)
        cls = G.class_counts(G.classify(bounds, grid))
        for v in variants(ctx):
            ctx.set_render_variant(v)
            t = new_planes(ctx, grid)
            st = ctx.grid_accumulate(grid, **t)
            ctx.set_render_variant(P.Context.VARIANT_AUTO)
            assert st == cls, (st, cls)
            assert torch.equal(t["counts"].view(-1), want_count), "counts differ"
            assert torch.equal(t["top"].view(-1), want_top), "top differs"
            assert torch.equal(t["bottom"].view(-1), want_bottom), "bottom differs"
        print(f"grid {grid}: {int(m.sum())} of {ref.shape[0]} records in {int((want_count > 0).sum())} of {w * h} cells, {cls}")
        assert int(m.sum()) > 0 and cls["batches_windowed" if cell == 4000 else "batches_direct"] > 0
        del want_top, want_bottom, want_count, t


# ---- 8. the resource ---------------------------------------------------------------------------------------------------------------
def test_resource_height_map_world_coordinates():
    import torch
    r = P.Renderer(160, 90)
    try:
        image = scenes.synth_stream(600_000)[0]
        las = P.HuffmanLasData.create(image)
        las.load_all(r)
        info = las.las_info()
        xyz, pts = las.points(r, world=True)
        xyz, pts = xyz.cpu().numpy(), pts.cpu().numpy()
        rec = np.zeros(len(pts), P.POINT_DTYPE)
        for k, n in enumerate(("x", "y", "z")):
            rec[n] = pts[:, k]
        rec["color"] = pts[:, 3].view(np.uint32)
        for which, clip_z, lo, hi in (("top", None, None, None), ("bottom", None, (200.0, 300.0), (800.0, 650.5)), ("top", (30.0, 45.0), (0.0, 0.0), (1000.0, 1000.0))):
            height, rgba, count, grid = las.height_map(r, 4.0, lo, hi, which, clip_z)
            want_grid = P.grid_from_world(info, (info.min[0], info.min[1]) if lo is None else lo, (info.max[0], info.max[1]) if hi is None else hi, 4.0)
            g = tuple(getattr(grid, n) for n, _ in N.Grid._fields_)
            assert g == tuple(getattr(want_grid, n) for n, _ in N.Grid._fields_) and g[2] == 4000
            clip = None if clip_z is None else P.box_from_world(info, (-np.inf, -np.inf, clip_z[0]), (np.inf, np.inf, clip_z[1]))
            clip = None if clip is None else (tuple(clip.min), tuple(clip.max))
            m, idx = G.cells_of(rec, g[:5], clip)
            if clip_z is not None:                                          # the integer clip is the float64 predicate's
                inz = (xyz[:, 2] >= clip_z[0]) & (xyz[:, 2] <= clip_z[1])
                assert np.array_equal(m, G.cells_of(rec, g[:5])[0] & inz)
            cells = g[3] * g[4]
            wz = np.full(cells, -np.inf if which == "top" else np.inf)
            (np.maximum if which == "top" else np.minimum).at(wz, idx, xyz[m, 2])       # float64 world heights: a monotone map of z
            wc = np.bincount(idx, minlength=cells)
            wz[wc == 0] = np.nan
            ref = G.reference(rec, g[:5], clip)
            _, wr = G.unpack(ref[0 if which == "top" else 1], G.EMPTY_TOP if which == "top" else G.EMPTY_BOTTOM)
            assert height.dtype == torch.float64 and tuple(height.shape) == (g[4], g[3]) and tuple(rgba.shape) == (g[4], g[3], 4)
            assert np.array_equal(height.cpu().numpy().ravel(), wz, equal_nan=True)
            assert np.array_equal(count.cpu().numpy().ravel(), wc.astype(np.int32))
            assert rgba.dtype == torch.uint8 and np.array_equal(rgba.cpu().numpy().reshape(-1, 4), wr.ravel().view(np.uint8).reshape(-1, 4))
            assert 0 < (wc > 0).sum() and (wc == 0).sum() + (wc > 0).sum() == cells
        with pytest.raises(ValueError):
            las.height_map(r, 0.0015)                                       # not a whole number of lattice steps
        with pytest.raises(ValueError):
            las.height_map(r, 4.0, which="middle")
    finally:
        r.ctx.close()


# ---- 9. the CLI --------------------------------------------------------------------------------------------------------------------
def run(*cmd):
    res = subprocess.run([str(c) for c in cmd], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    return res


def read_ppm(path):
    data = open(path, "rb").read()
    magic, dims, maxv, body = data.split(b"\n", 3)
    w, h = (int(v) for v in dims.split())
    assert magic == b"P6" and maxv == b"255" and len(body) == w * h * 3
    return np.frombuffer(body, np.uint8).reshape(h, w, 3)


def test_cli_ortho_round_trip(tmp_path):
    build.build_tools()
    image = scenes.synth_stream(600_000)[0]
    (tmp_path / "a.huffman").write_bytes(bytes(image.view()))
    info = P.HuffmanFile(image.view()).batch_las_info(0)
    c = P.Context(0)
    try:
        c.layout_name = "auto"
        load(c, image.view(), frame=False)
        box_lo, box_hi = (200.0, 300.0, 30.0), (800.5, 650.0, 45.0)
        for tag, extra, lo, hi, clip in (("all", [], (info.min[0], info.min[1]), (info.max[0], info.max[1]), None),
                                         ("box", ["--box", *(repr(v) for v in box_lo + box_hi)], box_lo[:2], box_hi[:2],
                                          P.box_from_world(info, (-np.inf, -np.inf, box_lo[2]), (np.inf, np.inf, box_hi[2])))):
            ppm, asc = tmp_path / f"{tag}.ppm", tmp_path / f"{tag}.asc"
            res = run(build.DECODE_BIN, tmp_path / "a.huffman", ppm, "--ortho", "4.0", *extra, "--dsm", asc)
            grid = P.grid_from_world(info, lo, hi, 4.0)
            top, _, count = c.read_grid(grid, clip)
            z, rgba = G.unpack(top, G.EMPTY_TOP)
            head = dict(line.split() for line in open(asc).read().split("\n")[:6])
            assert list(head) == ["ncols", "nrows", "xllcorner", "yllcorner", "cellsize", "NODATA_value"]
            assert (int(head["ncols"]), int(head["nrows"]), head["NODATA_value"]) == (grid.width, grid.height, "-9999")
            assert float(head["xllcorner"]) == grid.origin_x * info.scale[0] + info.offset[0] and float(head["cellsize"]) == 4.0
            assert float(head["yllcorner"]) == grid.origin_y * info.scale[1] + info.offset[1]
            want = np.where(count > 0, z.astype(np.float64) * info.scale[2] + info.offset[2], -9999.0)[::-1]
            got = np.loadtxt(asc, skiprows=6, ndmin=2)
            assert got.shape == want.shape and np.array_equal(got, want)     # %.17g round-trips a double
            img = read_ppm(ppm)
            assert np.array_equal(img, rgba.view(np.uint8).reshape(grid.height, grid.width, 4)[::-1, :, :3])
            assert 0 < (count > 0).sum() and "windowed" in res.stdout
        # without --dsm only the image is written
        run(build.DECODE_BIN, tmp_path / "a.huffman", tmp_path / "only.ppm", "--ortho", "4.0")
        assert open(tmp_path / "only.ppm", "rb").read() == open(tmp_path / "all.ppm", "rb").read()
        # without --ortho the tool does what it did: every point, as a LAS file
        run(build.DECODE_BIN, tmp_path / "a.huffman", tmp_path / "all.las")
        ax, ay, az, ac, alas = P.read_las(str(tmp_path / "all.las"))
        ref = c.read_points()
        assert np.array_equal(ax, ref["x"]) and np.array_equal(ay, ref["y"]) and np.array_equal(az, ref["z"]) and np.array_equal(ac, ref["color"])
        P.write_las(str(tmp_path / "ref.las"), points=ref, las=info)
        assert open(tmp_path / "all.las", "rb").read() == open(tmp_path / "ref.las", "rb").read()
        # a grid no point falls into is an error, not an empty image; a cell off the lattice too
        for extra, msg in ((["--box", "5000", "5000", "0", "6000", "6000", "100"], "no points"), (["--box", "0", "0", "5000", "1000", "1000", "6000"], "no points")):
            res = subprocess.run([str(build.DECODE_BIN), str(tmp_path / "a.huffman"), str(tmp_path / "none.ppm"), "--ortho", "4.0", *extra],
                                 stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
            assert res.returncode == 1 and msg in res.stderr and not (tmp_path / "none.ppm").exists()
        res = subprocess.run([str(build.DECODE_BIN), str(tmp_path / "a.huffman"), str(tmp_path / "none.ppm"), "--ortho", "0.0015"],
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert res.returncode == 1 and "lattice" in res.stderr and not (tmp_path / "none.ppm").exists()
    finally:
        c.close()
