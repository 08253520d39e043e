"""BC7 mode-6 colours (the reference built with COLOR_COMPRESSION == 7): the oracle's restatement of the
kernels' decode_bc7 against the reference's own BC7 encoder and decoder (tests/golden/bc7_ref_blocks.npz, made by
tools/make_golden.py through oracle/_ref), this repository's mode-6 encoder, the file format, and -- on the GPU -- the HQS
colour pass over a BC7 stream against the oracle."""
import os

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import _native as N
from tests import oracle, refpin, scenes

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WEIGHTS4 = [0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64]   # the specification's 4-bit weights


def spec_decode(block: np.ndarray, kernel_quirk: bool) -> np.ndarray:
    """BC7 mode 6 by the specification (independent of oracle/pcr_oracle.c); kernel_quirk: pixel 0 takes the 4-bit field at
    bit 0 of the high quadword -- (index << 1) | p1 -- as huffman_hqs/render.cu:262 does."""
    lo = int.from_bytes(block[:8].tobytes(), "little"); hi = int.from_bytes(block[8:].tobytes(), "little")
    assert lo & 0x7F == 0x40
    f = lambda sh: (lo >> sh) & 127
    p0, p1 = lo >> 63, hi & 1
    e0 = [(f(7) << 1) | p0, (f(21) << 1) | p0, (f(35) << 1) | p0, (f(49) << 1) | p0]
    e1 = [(f(14) << 1) | p1, (f(28) << 1) | p1, (f(42) << 1) | p1, (f(56) << 1) | p1]
    out = np.zeros(16, np.uint32)
    for i in range(16):
        idx = (hi >> 1) & 7 if i == 0 else (hi >> (4 * i)) & 15
        if i == 0 and kernel_quirk:
            idx = hi & 15
        w = WEIGHTS4[idx]
        ch = [((e0[c] * (64 - w) + e1[c] * w + 32) >> 6) & 255 for c in range(4)]
        out[i] = ch[0] | (ch[1] << 8) | (ch[2] << 16) | (ch[3] << 24)
    return out


def test_oracle_decode_follows_the_kernels_and_the_reference_decoder():
    d = np.load(os.path.join(G, "bc7_ref_blocks.npz"))
    blocks, unpacked = d["blocks"], d["unpacked"]
    flat = np.ascontiguousarray(blocks.reshape(-1))
    differ0 = 0
    for k in range(len(blocks)):
        got = np.array([oracle.decode_bc7(16 * k + i, flat) for i in range(16)], np.uint32)
        assert np.array_equal(got, spec_decode(blocks[k], kernel_quirk=True))
        # pixels 1..15: what the reference's own CPU decoder (src/bc7decomp.cpp) unpacks; pixel 0: the kernels read one bit
        # too many there (render.cu:262), so it may differ from the specification -- reproduced, and counted
        assert np.array_equal(got[1:], unpacked[k][1:])
        assert np.array_equal(spec_decode(blocks[k], kernel_quirk=False), unpacked[k])
        differ0 += int(got[0] != unpacked[k][0])
    assert 0 < differ0 < len(blocks)


def test_reference_library_reproduces_the_committed_blocks():
    if not os.path.exists(oracle.REF_LIB):
        pytest.skip("oracle/_ref not built (the reference checkout is absent)")
    d = np.load(os.path.join(G, "bc7_ref_blocks.npz"))
    ref = refpin.ref_lib()
    # the arrays are read once and held: d["colors"] reads the file anew at every access, and a temporary's `.ctypes.data` is the
    # address of memory that is freed before the call is made
    colors, blocks, unpacked = (np.ascontiguousarray(d[n]) for n in ("colors", "blocks", "unpacked"))
    assert colors.dtype == np.uint32 and colors.shape[1] == 16
    for k in range(0, len(colors), 7):
        enc = np.zeros(16, np.uint8); unp = np.zeros(16, np.uint32)
        row = colors[k]
        ref.ref_bc7_encode(row.ctypes.data, enc.ctypes.data)
        assert ref.ref_bc7_unpack(enc.ctypes.data, unp.ctypes.data) == 1
        assert np.array_equal(enc, blocks[k]) and np.array_equal(unp, unpacked[k])


def psnr(a: np.ndarray, b: np.ndarray) -> float:
    ch = lambda v: np.stack([(v >> s) & 255 for s in (0, 8, 16)], -1).astype(np.float64)
    mse = ((ch(a) - ch(b)) ** 2).mean()
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def test_own_encoder_writes_valid_mode6_blocks_of_reference_quality():
    d = np.load(os.path.join(G, "bc7_ref_blocks.npz"))
    colors = d["colors"]
    mine = np.zeros((len(colors), 16), np.uint8)
    for k in range(len(colors)):
        N.host_lib().pcr_bc7_encode_block(np.ascontiguousarray(colors[k]).ctypes.data, mine[k].ctypes.data)
        assert mine[k][0] & 0x7F == 0x40                                    # mode 6
    dec_mine = np.stack([spec_decode(b, kernel_quirk=False) for b in mine])
    if os.path.exists(oracle.REF_LIB):                                      # the reference's decoder accepts them
        ref = refpin.ref_lib()
        for k in range(0, len(mine), 5):
            unp = np.zeros(16, np.uint32)
            assert ref.ref_bc7_unpack(mine[k].ctypes.data, unp.ctypes.data) == 1
            assert np.array_equal(unp, dec_mine[k])
    mine_db, ref_db = psnr(dec_mine, colors), psnr(d["unpacked"], colors)
    assert mine_db > ref_db - 3.0, (mine_db, ref_db)                        # a bounding-box encoder: within 3 dB of bc7enc


def bc7_stream(n=150_000, seed=11):
    x, y, z, c = P.synth_points(n, seed, 0, n)
    las = P.synth_las_info(n, seed)
    return P.encode_points(x, y, z, c, las, morton_sort=True, nthreads=2, bc7=True)


def test_file_format_and_oracle_colour_pass():
    nb, st = bc7_stream()
    nb1, _ = P.encode_points(*P.synth_points(150_000, 11, 0, 150_000), P.synth_las_info(150_000, 11), morton_sort=True, nthreads=2)
    of, of1 = oracle.OracleFile(nb.view()), oracle.OracleFile(nb1.view())
    assert of.s.color_format == 7 and of1.s.color_format in (0, 1)
    assert len(nb.view()) - len(nb1.view()) == of.num_batches * 32768       # 16 instead of 8 colour bytes per 16 points
    f = P.HuffmanFile(nb)
    assert f.numBatches == of.num_batches
    p = scenes.cameras(320, 200)["overview"]
    fb, _ = of.render_hqs_depth(p); fb1, _ = of1.render_hqs_depth(p)
    assert np.array_equal(fb, fb1)                                          # same points
    rg, ba, _ = of.render_hqs_color(p, fb); rg1, ba1, _ = of1.render_hqs_color(p, fb1)
    assert np.array_equal(ba & 0xFFFFFFFF, ba1 & 0xFFFFFFFF)                # same counts
    img, img1 = oracle.resolve_hqs(p, fb, rg, ba), oracle.resolve_hqs(p, fb1, rg1, ba1)
    covered = (fb[:320 * 200] >> 32) != 0xFFFFFFFF
    assert covered.sum() > 1000 and psnr(img[covered], img1[covered]) > 25.0   # the two codecs show the same picture


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["point_windows", "words"])
def test_hqs_draws_a_bc7_stream_like_the_oracle(layout):
    nb, _ = bc7_stream(400_000, seed=5)
    of = oracle.OracleFile(nb.view())
    r = P.Renderer(640, 360, device=0)
    try:
        ctx = r.ctx
        ctx.set_stream_layout(P.Context.LAYOUT_POINT_WINDOWS if layout == "point_windows" else P.Context.LAYOUT_WORDS)
        las = P.HuffmanLasData.create(nb)
        las.load_all(r)
        assert ctx.stream_color_format() == 7
        for cam in ("overview", "closeup"):
            for lod in (10, 100):
                p = scenes.with_flags(scenes.cameras(640, 360)[cam], lod_percent=lod)
                ctx.clear(); ctx.render_hqs_depth(p)
                hfb, hst = of.render_hqs_depth(p)
                assert ctx.stats() == hst and np.array_equal(ctx.read_framebuffer(full=True), hfb)
                ctx.render_hqs_color(p); ctx.resolve_hqs(p)
                org, oba, _ = of.render_hqs_color(p, hfb)
                rg, ba = ctx.read_accum(full=True)
                assert np.array_equal(rg, org) and np.array_equal(ba, oba)
                assert np.array_equal(ctx.read_rgba(), oracle.resolve_hqs(p, hfb, org, oba))
        with pytest.raises(P.PcrError, match="BC7"):                        # the reference's basic method has no defined BC7 result
            ctx.render_basic(scenes.cameras(640, 360)["overview"])
    finally:
        r.ctx.close()


@pytest.mark.gpu
def test_bc7_stream_through_the_asynchronous_loader():
    """The first records of a BC7 stream make the context re-allocate its colour arrays (they were sized for BC1); with
    pcr_set_async_upload the copies and k_transcode run on the loader stream, so the zero fill of the new arrays has to be
    behind them before they start: the colours of the first loader task would otherwise be wiped."""
    import time
    nb, _ = bc7_stream(1_500_000, seed=9)                                   # 23 batches
    of = oracle.OracleFile(nb.view())
    hf = P.HuffmanFile(nb)
    ctx = P.Context(0)
    try:
        ctx.set_image_size(640, 360)
        ctx.stream_begin(hf.header())
        ctx.set_async_upload(True)
        for b0 in range(0, hf.numBatches, 8):
            ctx.upload_batches(b0, [hf.blob(b) for b in range(b0, min(b0 + 8, hf.numBatches))])
        t0 = time.time()
        while ctx.batches_resident < hf.numBatches:
            assert time.time() - t0 < 30.0, "loader stream made no progress"
            time.sleep(0.001)
        assert ctx.stream_color_format() == 7
        p = scenes.with_flags(scenes.cameras(640, 360)["overview"], lod_percent=100)
        ctx.clear(); ctx.render_hqs_depth(p); ctx.render_hqs_color(p); ctx.resolve_hqs(p)
        hfb, _ = of.render_hqs_depth(p)
        org, oba, _ = of.render_hqs_color(p, hfb)
        rg, ba = ctx.read_accum(full=True)
        assert np.array_equal(ctx.read_framebuffer(full=True), hfb)
        assert np.array_equal(rg, org) and np.array_equal(ba, oba)
        assert np.array_equal(ctx.read_rgba(), oracle.resolve_hqs(p, hfb, org, oba))
    finally:
        ctx.set_async_upload(False)
        ctx.close()
