"""The numpy side of the display-resolve tests (pcr_resolve_*_display): include/pcr_hip.h's three steps restated operation by
operation, and the cases tests/test_display_cpu.py and tests/test_gpu_display.py share. Inputs and reference arithmetic only.

Every reference image is computed from a framebuffer of the CPU ORACLE. The window-only image is exact: the dilation is the
unsigned 64-bit minimum over the clipped window, taken offset by offset (not separably, as the kernel does), the colour goes
through the oracle's own resolve arithmetic, the 1 % test of the HQS colour is one np.float32 product. The eye-dome-lighting
image is evaluated in float64 (edl(..., dtype=np.float32) is the same formula in the kernel's precision)."""
from __future__ import annotations

import functools

import numpy as np

import pcrhpg24_amd as P
from tests import oracle, scenes

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
BACKGROUND = 0x00443322
TOTAL_POINTS = 8 * 65536
WINDOWS = (1, 2, 4)
SIZES = ((320, 200), (333, 77), (67, 19))           # the sizes the preconditions are checked at
EDL_WINDOWS = (1, 2)
EDL_STRENGTHS = (0.0005, 0.02)


def stream():
    return scenes.synth_stream(TOTAL_POINTS)[0]


@functools.lru_cache(maxsize=None)
def oracle_file() -> oracle.OracleFile:
    return oracle.OracleFile(stream().view())


def camera(name: str, W: int, H: int, **flags) -> P.RenderParams:
    return scenes.with_flags(scenes.cameras(W, H)[name], lod_percent=100, cull=1, **flags)


def opts(window: int = 0, edl_window: int = 0, strength: float = 0.0, reserved: int = 0) -> P.DisplayOpts:
    o = P.DisplayOpts()
    o.window, o.edl_window, o.edl_strength, o.reserved = window, edl_window, strength, reserved
    return o


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def basic_frame(cam: str, W: int, H: int, show_num_points: int = 0, colorize_chunks: int = 0):
    """(params, fb) of the oracle's basic frame; fb has pcr_fb_elems words and is read-only."""
    p = camera(cam, W, H, show_num_points=show_num_points, colorize_chunks=colorize_chunks)
    fb, _ = oracle_file().render_basic(p)
    return (p,) + _frozen(fb)


def hqs_frame_of(of: oracle.OracleFile, p: P.RenderParams):
    fb, _ = of.render_hqs_depth(p)
    rg, ba, _ = of.render_hqs_color(p, fb)
    return _frozen(fb, rg, ba)


@functools.lru_cache(maxsize=None)
def hqs_frame(cam: str, W: int, H: int, show_num_points: int = 0, colorize_chunks: int = 0):
    """(params, fb, rg, ba) of the oracle's HQS frame, read-only."""
    p = camera(cam, W, H, show_num_points=show_num_points, colorize_chunks=colorize_chunks)
    return (p,) + hqs_frame_of(oracle_file(), p)


# ---- step 1: the dilated word ---------------------------------------------------------------------------------------------------
def _padded(a: np.ndarray, r: int, fill):
    H, W = a.shape
    out = np.full((H + 2 * r, W + 2 * r), fill, a.dtype)
    out[r:r + H, r:r + W] = a
    return out


def offsets(r: int):
    """The (ox, oy) of a window of radius r in the order of the contract's EDL sum: ox outer, oy inner."""
    return [(ox, oy) for ox in range(-r, r + 1) for oy in range(-r, r + 1)]


def shifted(pad: np.ndarray, r: int, ox: int, oy: int, H: int, W: int):
    """pad[y + oy, x + ox] for every pixel (x, y) of the image, pad = _padded(image, r, ...)."""
    return pad[r + oy:r + oy + H, r + ox:r + ox + W]


def dilate(fb: np.ndarray, W: int, H: int, w: int) -> np.ndarray:
    """D[y, x] = the unsigned 64-bit minimum of the frame's words over the window of radius w, clipped to the image."""
    f = np.asarray(fb[:W * H], np.uint64).reshape(H, W)
    pad = _padded(f, w, EMPTY)
    out = f.copy()
    for ox, oy in offsets(w):
        out = np.minimum(out, shifted(pad, w, ox, oy, H, W))
    return out


def depth_of(words: np.ndarray) -> np.ndarray:
    return (np.asarray(words, np.uint64) >> np.uint64(32)).astype(np.uint32).view(np.float32)


# ---- step 2: the colour -----------------------------------------------------------------------------------------------------------
def basic_image(p, fb, w: int) -> np.ndarray:
    D = dilate(fb, p.width, p.height, w)
    return oracle.resolve_basic(p, np.ascontiguousarray(D).ravel()).reshape(p.height, p.width), D


def las_image(p, fb, rgba_points, w: int):
    D = dilate(fb, p.width, p.height, w)
    return oracle.resolve_las(p, np.ascontiguousarray(D).ravel(), rgba_points).reshape(p.height, p.width), D


def hqs_sums(p, fb, rg, ba, w: int):
    """(D, RG', BA', accepted, rejected): the sums over the window's pixels that are drawn and whose own depth d_n <= d * 1.01f, d
    the depth of D (np.float32 product), and per pixel how many drawn neighbours passed / failed that test."""
    W, H = p.width, p.height
    D = dilate(fb, W, H, w)
    with np.errstate(invalid="ignore"):
        limit = depth_of(D) * np.float32(1.01)
        assert limit.dtype == np.float32
        pfb = _padded(np.asarray(fb[:W * H], np.uint64).reshape(H, W), w, EMPTY)
        prg = _padded(np.asarray(rg[:W * H], np.uint64).reshape(H, W), w, np.uint64(0))
        pba = _padded(np.asarray(ba[:W * H], np.uint64).reshape(H, W), w, np.uint64(0))
        RG, BA = np.zeros((H, W), np.uint64), np.zeros((H, W), np.uint64)
        accepted, rejected = np.zeros((H, W), np.int32), np.zeros((H, W), np.int32)
        for ox, oy in offsets(w):
            n = shifted(pfb, w, ox, oy, H, W)
            drawn = n != EMPTY
            ok = drawn & (depth_of(n) <= limit)
            RG += np.where(ok, shifted(prg, w, ox, oy, H, W), np.uint64(0))
            BA += np.where(ok, shifted(pba, w, ox, oy, H, W), np.uint64(0))
            accepted += ok
            rejected += drawn & ~ok
    drawn_c = D != EMPTY
    return D, RG, BA, np.where(drawn_c, accepted, 0), np.where(drawn_c, rejected, 0)


def hqs_image(p, fb, rg, ba, w: int):
    D, RG, BA, _, _ = hqs_sums(p, fb, rg, ba, w)
    img = oracle.resolve_hqs(p, np.ascontiguousarray(D).ravel(), np.ascontiguousarray(RG).ravel(), np.ascontiguousarray(BA).ravel())
    return img.reshape(p.height, p.width), D


# ---- step 3: eye-dome lighting ----------------------------------------------------------------------------------------------------
def edl(img: np.ndarray, D: np.ndarray, e: int, strength: float, dtype=np.float64):
    """(shaded image, response): step 3 on the dilated words D, every operation in `dtype`. The strength is the f32 the call is
    given. Pixels with an empty D keep their colour; their response is 0."""
    H, W = D.shape
    drawn = D != EMPTY
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.where(drawn, depth_of(D), np.float32(0)).astype(dtype)
        pd, pv = _padded(d, e, dtype(0)), _padded(drawn, e, False)
        total = np.zeros((H, W), dtype)
        for ox, oy in offsets(e):
            t = np.where(shifted(pv, e, ox, oy, H, W), np.maximum(dtype(0), d - shifted(pd, e, ox, oy, H, W)), dtype(0))
            total = total + t
        response = np.where(drawn, total / dtype((2 * e + 1) * (2 * e + 1)), dtype(0))
        shade = np.exp((-response * dtype(300.0)) * dtype(np.float32(strength)))
        assert response.dtype == dtype and shade.dtype == dtype
        out = np.zeros((H, W), np.uint32)
        for k in range(3):
            byte = ((img >> np.uint32(8 * k)) & np.uint32(255)).astype(dtype)
            out |= (byte * shade).astype(np.uint32) << np.uint32(8 * k)
    return np.where(drawn, out, img).astype(np.uint32), response


def channels(img: np.ndarray) -> np.ndarray:
    """[..., 4] int32 bytes of an RGBA8 image."""
    return np.stack([(np.asarray(img, np.uint32) >> np.uint32(8 * k)) & np.uint32(255) for k in range(4)], axis=-1).astype(np.int32)


def edl_check(got: np.ndarray, ref: np.ndarray, response: np.ndarray, D: np.ndarray):
    """The EDL expectations of the issue, on a GPU (or float32) image against the float64 one: every channel within 1, pixels
    of response 0 (all background among them) equal, at most 1 % of the drawn pixels different at all. Returns the count."""
    got, ref = np.asarray(got, np.uint32).reshape(ref.shape), np.asarray(ref, np.uint32)
    diff = np.abs(channels(got) - channels(ref)).max(axis=-1)
    assert diff.max() <= 1, f"a channel is off by {diff.max()} at {np.argwhere(diff > 1)[:4]}"
    flat = response == 0
    assert np.array_equal(got[flat], ref[flat]), "a pixel of response 0 differs"
    drawn = int((D != EMPTY).sum())
    differing = int((diff > 0).sum())
    assert differing * 100 <= drawn, f"{differing} of {drawn} drawn pixels differ"
    return differing


# ---- the independent formulation of step 1: squares drawn with a 64-bit minimum ----------------------------------------------
def splat_squares(pix, depth, colour, W: int, H: int, w: int) -> np.ndarray:
    """Every traced point's depth << 32 | colour drawn into the (2w+1)^2 square around its pixel, clipped to the image, with
    np.minimum.at; points whose row is >= H (the framebuffer's spare row) are dropped."""
    pix = np.asarray(pix, np.int64)
    key = (np.asarray(depth, np.uint64) << np.uint64(32)) | np.asarray(colour, np.uint64)
    x, y = pix % W, pix // W
    keep = y < H
    x, y, key = x[keep], y[keep], key[keep]
    out = np.full(W * H, EMPTY, np.uint64)
    for ox, oy in offsets(w):
        tx, ty = x + ox, y + oy
        m = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
        np.minimum.at(out, ty[m] * W + tx[m], key[m])
    return out.reshape(H, W)
