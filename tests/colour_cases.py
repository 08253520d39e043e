"""Constructed BC1 / BC7 colour blocks, the streams that carry them and the decode rule restated in numpy (tests/test_colour_cpu.py
asserts on the CPU what the block sets cover and holds the restatement against the oracle, the fixtures and the reference's decoder;
tests/test_gpu_colour.py holds every kernel that decodes a colour against it). Inputs and the reference only, no expectations of the GPU.

The geometry of every stream is the same: a batch is a 256 x 256 lattice of points 1000 lattice steps apart on z = 0, the batches lie
side by side as tiles, and the stream is encoded unsorted with padded tails, so record r of batch t is lattice point (r % 256, r // 256)
of tile t. The encoder's own colour blocks -- the last 32 768 (BC1) or 65 536 (BC7) bytes of every batch record -- are then overwritten
with the constructed ones: block k of a batch colours its records 16 k .. 16 k + 15.

  bc1_all    4 exhaustive batches, the special batch, a random batch
  bc7_all    32 exhaustive batches, the special batch, a random batch
  bc7_frame  the special batch, the first batch of either exhaustive half, the random batch (for the frames)"""
from __future__ import annotations

import functools
import os

import numpy as np

import pcrhpg24_amd as P
from tests import scenes

PPB = 65536
BLOCKS = PPB // 16                                  # colour blocks of a batch
SIDE, STEP = 256, 1000                              # lattice points per tile edge, lattice steps between them
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WEIGHTS4 = np.array([0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64], np.int64)    # the specification's 4-bit weights
STREAMS = ("bc1_all", "bc7_all", "bc7_frame")


# ---- the decode rule ----------------------------------------------------------------------------------------------------------------
def spec_bc1(blocks) -> np.ndarray:
    """uint32 [n, 16], 0x00BBGGRR of the 16 pixels of n BC1 blocks (uint8, 8 bytes each): 5/6-bit endpoints expanded by bit
    replication, the palette e0, e1, (2 e0 + e1) // 3, (e0 + 2 e1) // 3 whatever the order of the endpoints, pixel l picks the entry
    named by bits 2 l of the high dword."""
    b = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 8).astype(np.int64)
    c = [b[:, 0] | b[:, 1] << 8, b[:, 2] | b[:, 3] << 8]
    sel = (b[:, 4] | b[:, 5] << 8 | b[:, 6] << 16 | b[:, 7] << 24)[:, None] >> (2 * np.arange(16, dtype=np.int64))[None, :] & 3
    out = np.zeros((len(b), 16), np.int64)
    for shift, (at, bits) in zip((0, 8, 16), ((11, 5), (5, 6), (0, 5))):                        # r, g, b of 565
        f = [(w >> at) & ((1 << bits) - 1) for w in c]
        e0, e1 = (v << (8 - bits) | v >> (2 * bits - 8) for v in f)
        palette = np.stack([e0, e1, (2 * e0 + e1) // 3, (e0 + 2 * e1) // 3], axis=1)
        out |= np.take_along_axis(palette, sel, axis=1) << shift
    return out.astype(np.uint32)


def bc7_quadwords(blocks):
    q = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 16).view("<u8")
    return q[:, 0].copy(), q[:, 1].copy()


def spec_bc7(blocks) -> np.ndarray:
    """uint32 [n, 16], 0xAABBGGRR of the 16 pixels of n BC7 blocks (uint8, 16 bytes each) as the renderers read them: mode-6 fields
    whatever the mode bits say, endpoint = 7-bit field << 1 | p (p0: bit 63 of the low quadword, p1: bit 0 of the high one), the index
    of pixel l the 4-bit field at 4 l of the high quadword for EVERY l, channel = (E0 (64 - w) + E1 w + 32) >> 6."""
    lo, hi = bc7_quadwords(blocks)
    field = lambda q, at, bits: ((q >> np.uint64(at)) & np.uint64((1 << bits) - 1)).astype(np.int64)
    p0, p1 = field(lo, 63, 1), field(hi, 0, 1)
    idx = np.stack([field(hi, 4 * l, 4) for l in range(16)], axis=1)
    w = WEIGHTS4[idx]
    out = np.zeros((len(lo), 16), np.int64)
    for ch in range(4):
        e0 = (field(lo, 7 + 14 * ch, 7) << 1 | p0)[:, None]
        e1 = (field(lo, 14 + 14 * ch, 7) << 1 | p1)[:, None]
        out |= ((e0 * (64 - w) + e1 * w + 32) >> 6) << (8 * ch)
    return out.astype(np.uint32)


# ---- the fields of built bytes (for the coverage counts) ------------------------------------------------------------------------------
def bc1_fields(blocks):
    """c0, c1 (the 16-bit endpoint words), and per channel r, g, b the raw (e0, e1) fields; selectors int64 [n, 16]."""
    b = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 8).astype(np.int64)
    c0, c1 = b[:, 0] | b[:, 1] << 8, b[:, 2] | b[:, 3] << 8
    sel = (b[:, 4] | b[:, 5] << 8 | b[:, 6] << 16 | b[:, 7] << 24)[:, None] >> (2 * np.arange(16, dtype=np.int64))[None, :] & 3
    ch = {"r": ((c0 >> 11) & 31, (c1 >> 11) & 31), "g": ((c0 >> 5) & 63, (c1 >> 5) & 63), "b": (c0 & 31, c1 & 31)}
    return c0, c1, ch, sel


def bc7_fields(blocks):
    """mode (the low seven bits), per channel r, g, b, a the 8-bit endpoints (E0, E1), and the 4-bit fields int64 [n, 16]."""
    lo, hi = bc7_quadwords(blocks)
    field = lambda q, at, bits: ((q >> np.uint64(at)) & np.uint64((1 << bits) - 1)).astype(np.int64)
    p0, p1 = field(lo, 63, 1), field(hi, 0, 1)
    ch = {n: (field(lo, 7 + 14 * k, 7) << 1 | p0, field(lo, 14 + 14 * k, 7) << 1 | p1) for k, n in enumerate("rgba")}
    return field(lo, 0, 7), ch, np.stack([field(hi, 4 * l, 4) for l in range(16)], axis=1)


# ---- BC1 block sets -------------------------------------------------------------------------------------------------------------------
def pack_bc1(c0, c1, selectors) -> np.ndarray:
    """uint8 [n, 8] from the endpoint words and the 32-bit selector words."""
    out = np.zeros((len(c0), 2), "<u4")
    out[:, 0] = np.asarray(c0, np.int64) | np.asarray(c1, np.int64) << 16
    out[:, 1] = np.asarray(selectors, np.int64)
    return out.view(np.uint8).reshape(-1, 8)


def selector_word(sel) -> np.ndarray:
    """The 32-bit word of selectors int64 [n, 16] (pixel l at bits 2 l)."""
    return (np.asarray(sel, np.int64) << (2 * np.arange(16, dtype=np.int64))[None, :]).sum(axis=1)


def bc1_exhaustive() -> np.ndarray:
    """4 batches: every (e0, e1, selector) of every channel, every selector at every local position; c0 < c1 and c0 == c1 included."""
    k = np.arange(BLOCKS, dtype=np.int64)
    g0, g1 = k >> 6, k & 63
    r0, r1 = k & 31, (k >> 5) & 31
    b0, b1 = (k >> 7) & 31, (k >> 2) & 31
    c0, c1 = r0 << 11 | g0 << 5 | b0, r1 << 11 | g1 << 5 | b1
    out = []
    for s in range(4):
        sel = np.broadcast_to((np.arange(16, dtype=np.int64) + s) & 3, (BLOCKS, 16))
        out.append(pack_bc1(c0, c1, selector_word(sel)))
    return np.concatenate(out)


def golden_blocks(name: str) -> np.ndarray:
    return np.ascontiguousarray(np.load(os.path.join(G, name))["blocks"], np.uint8)


def bc1_special() -> np.ndarray:
    """1 batch: 1024 random blocks with c0 == c1; 1024 random blocks with c0 < c1 and selector 3 everywhere (a standard decoder's
    transparent black); the {0x0000, 0xFFFF}^2 endpoints under the four uniform selector words; the reference encoder's 256 blocks;
    random 64-bit blocks."""
    rng = np.random.default_rng(101)
    same = rng.integers(0, 1 << 16, 1024)
    a, b = rng.integers(0, 1 << 16, (2, 1024))
    b = np.where(a == b, a ^ 1, b)
    parts = [pack_bc1(same, same, rng.integers(0, 1 << 32, 1024)),
             pack_bc1(np.minimum(a, b), np.maximum(a, b), np.full(1024, 0xFFFFFFFF))]
    ends = np.array([(x, y) for x in (0, 0xFFFF) for y in (0, 0xFFFF)], np.int64)
    for word in (0x00000000, 0x55555555, 0xAAAAAAAA, 0xFFFFFFFF):
        parts.append(pack_bc1(ends[:, 0], ends[:, 1], np.full(4, word)))
    parts.append(golden_blocks("bc1_ref_blocks.npz").reshape(-1, 8))
    used = sum(len(p) for p in parts)
    parts.append(rng.integers(0, 256, (BLOCKS - used, 8)).astype(np.uint8))
    return np.concatenate(parts)


def bc1_random() -> np.ndarray:
    return np.random.default_rng(102).integers(0, 256, (BLOCKS, 8)).astype(np.uint8)


# ---- BC7 block sets -------------------------------------------------------------------------------------------------------------------
def pack_bc7(mode, fields, p0, p1, index_fields) -> np.ndarray:
    """uint8 [n, 16]: fields int64 [n, 8] (r0 r1 g0 g1 b0 b1 a0 a1, 7 bits each), index_fields int64 [n, 16], 4 bits each, of which
    bit 0 of pixel 0's is p1 and is taken from p1."""
    n = len(p0)
    lo = np.asarray(mode, np.int64).astype(np.uint64) & np.uint64(127)
    for j in range(8):
        lo |= fields[:, j].astype(np.uint64) << np.uint64(7 + 7 * j)
    lo |= np.asarray(p0, np.int64).astype(np.uint64) << np.uint64(63)
    hi = np.zeros(n, np.uint64)
    for l in range(16):
        f = index_fields[:, l].astype(np.uint64) & np.uint64(15)
        if l == 0:
            f = (f & np.uint64(14)) | np.asarray(p1, np.int64).astype(np.uint64)
        hi |= f << np.uint64(4 * l)
    return np.stack([lo, hi], axis=1).astype("<u8").view(np.uint8).reshape(-1, 16)


def reverse7(f):
    f = np.asarray(f, np.int64)
    return sum(((f >> k) & 1) << (6 - k) for k in range(7))


def bc7_exhaustive() -> np.ndarray:
    """32 batches, two halves of 65 536 mode-6 blocks: block K has the red endpoints E0 = K & 255, E1 = K >> 8 (field = E >> 1, the
    p-bits are the low bits: they are shared by all channels), green the bit-reversed 7-bit fields, blue the complemented ones, alpha
    the fields xor 0x55; pixels 1 .. 15 hold the indices l in the first half and (l + 1) & 15 in the second, so every (E0, E1, index)
    occurs in every channel at a pixel that obeys the specification; the three upper bits of pixel 0's field go through all eight
    values."""
    K = np.arange(1 << 16, dtype=np.int64)
    e0, e1 = K & 255, K >> 8
    f0, f1, p0, p1 = e0 >> 1, e1 >> 1, e0 & 1, e1 & 1
    fields = np.stack([f0, f1, reverse7(f0), reverse7(f1), 127 - f0, 127 - f1, f0 ^ 0x55, f1 ^ 0x55], axis=1)
    out = []
    for half in range(2):
        idx = np.broadcast_to((np.arange(16, dtype=np.int64) + half) & 15, (len(K), 16)).copy()
        idx[:, 0] = (((K >> 1) if half == 0 else (K >> 9)) & 7) << 1
        out.append(pack_bc7(np.full(len(K), 0x40), fields, p0, p1, idx))
    return np.concatenate(out)


def with_pbits(blocks, p0: int, p1: int) -> np.ndarray:
    b = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 16).copy()
    b[:, 7] = (b[:, 7] & 0x7F) | (p0 << 7)
    b[:, 8] = (b[:, 8] & 0xFE) | p1
    return b


def bc7_special() -> np.ndarray:
    """1 batch: the reference encoder's 256 blocks; the same with each of the four (p0, p1); all zeros, all ones; random 128-bit
    blocks, mode bits and all."""
    ref = golden_blocks("bc7_ref_blocks.npz").reshape(-1, 16)
    parts = [ref] + [with_pbits(ref, p0, p1) for p0 in (0, 1) for p1 in (0, 1)]
    parts += [np.zeros((1, 16), np.uint8), np.full((1, 16), 255, np.uint8)]
    used = sum(len(p) for p in parts)
    parts.append(np.random.default_rng(103).integers(0, 256, (BLOCKS - used, 16)).astype(np.uint8))
    return np.concatenate(parts)


def bc7_random() -> np.ndarray:
    return np.random.default_rng(104).integers(0, 256, (BLOCKS, 16)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def blocks(name: str) -> np.ndarray:
    """The blocks of a stream, uint8 [batches * 4096, 8 or 16], read-only."""
    if name == "bc1_all":
        out = np.concatenate([bc1_exhaustive(), bc1_special(), bc1_random()])
    elif name == "bc7_all":
        out = np.concatenate([bc7_exhaustive(), bc7_special(), bc7_random()])
    elif name == "bc7_frame":
        ex = bc7_exhaustive()
        out = np.concatenate([bc7_special(), ex[:BLOCKS], ex[16 * BLOCKS:17 * BLOCKS], bc7_random()])
    else:
        raise KeyError(name)
    assert len(out) % BLOCKS == 0
    out.setflags(write=False)
    return out


# (first batch, batches) of the parts of the two whole streams
PARTS = {"bc1_all": {"exhaustive": (0, 4), "special": (4, 1), "random": (5, 1)},
         "bc7_all": {"exhaustive": (0, 32), "special": (32, 1), "random": (33, 1)}}


def part(name: str, which: str) -> np.ndarray:
    first, count = PARTS[name][which]
    return blocks(name)[first * BLOCKS:(first + count) * BLOCKS]


def is_bc7(name: str) -> bool:
    return name.startswith("bc7")


def num_batches(name: str) -> int:
    return len(blocks(name)) // BLOCKS


@functools.lru_cache(maxsize=None)
def spec_colours(name: str) -> np.ndarray:
    """uint32 [records]: the colour of every record of the stream by the restated rule (BC7: alpha in bits 24 .. 31)."""
    out = (spec_bc7 if is_bc7(name) else spec_bc1)(blocks(name)).reshape(-1)
    out.setflags(write=False)
    return out


# ---- the streams ----------------------------------------------------------------------------------------------------------------------
def tiles(name: str) -> tuple[int, int]:
    """(columns, rows) of the tile layout: as square as the batch count allows, the last row may be short."""
    n = num_batches(name)
    cols = int(np.ceil(np.sqrt(n)))
    return cols, -(-n // cols)


@functools.lru_cache(maxsize=None)
def points(name: str) -> np.ndarray:
    """int32 [records, 3]: the input, which is what every record decodes to."""
    cols, _ = tiles(name)
    r = np.arange(PPB, dtype=np.int64)
    out = np.zeros((num_batches(name), PPB, 3), np.int32)
    for t in range(num_batches(name)):
        out[t, :, 0] = ((t % cols) * SIDE + r % SIDE) * STEP
        out[t, :, 1] = ((t // cols) * SIDE + r // SIDE) * STEP
    out = out.reshape(-1, 3)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def stream(name: str) -> bytes:
    """The .huffman image of the stream: the lattice encoded as given, the constructed blocks in place of the encoder's."""
    xyz, bc7 = points(name), is_bc7(name)
    x, y, z = (np.ascontiguousarray(xyz[:, k]) for k in range(3))
    c = np.random.default_rng(12).integers(0, 1 << 24, len(xyz)).astype(np.uint32)
    las = scenes.lattice_las((0, 0, 0), tuple(int(v) for v in xyz.max(axis=0)))
    native, st = P.encode_points(x, y, z, c, las, morton_sort=False, nthreads=2, pad_tails=True, bc7=bc7)
    assert st["num_batches"] == num_batches(name)
    image = np.frombuffer(native.view(), np.uint8).copy()
    nbytes = BLOCKS * (16 if bc7 else 8)
    ends = P.HuffmanFile(image).batch_offsets[1:]
    flat = blocks(name).reshape(-1)
    for b, end in enumerate(ends):                      # the colour array ends the batch record
        image[int(end) - nbytes:int(end)] = flat[b * nbytes:(b + 1) * nbytes]
    return image.tobytes()


# ---- the oracle's walk --------------------------------------------------------------------------------------------------------------
def walk_order(nb: int, npr: int = 64) -> np.ndarray:
    """The record of every entry of a whole-stream trace: the oracle walks a batch cluster by cluster (32 chains), point by point
    (the first npr of a chain), lane by lane."""
    b, c, i, l = np.meshgrid(np.arange(nb), np.arange(32), np.arange(npr), np.arange(32), indexing="ij")
    return (b * PPB + (c * 32 + l) * 64 + i).reshape(-1)


# ---- cameras --------------------------------------------------------------------------------------------------------------------------
PIXELS_PER_TILE = 384                                   # 1.5 pixels per lattice point
# The height from which a tile row -- 256 lattice steps with half a step around it -- just fills the image's rows at fovy 60:
# 128 / tan 30 = 221.7, rounded up. From higher up the lattice leaves a margin, and at 1 / 16 of the size the pixels on the image's
# border hold a few records only (from 230 a corner pixel of a 2 x 2 layout holds one).
RADIUS_PER_ROW = 222.0


def _camera(name: str, divide: int) -> P.RenderParams:
    cols, rows = tiles(name)
    target = ((cols * SIDE - 1) / 2.0, (rows * SIDE - 1) / 2.0, 0.0)
    return scenes.straight_down(RADIUS_PER_ROW * rows, target, cols * PIXELS_PER_TILE // divide, rows * PIXELS_PER_TILE // divide)


def one_per_pixel(name: str) -> P.RenderParams:
    """Straight down over the tiles, 1.5 pixels per lattice step: every record has a pixel of its own, all at one depth. (A batch is
    hundreds of pixels wide: its chains are drawn whole whatever lod_percent says, on the double-precision path.)"""
    return _camera(name, 1)


def many_per_pixel(name: str) -> P.RenderParams:
    """The same view at 1/16 of the width and height: 100 to 121 records per pixel, all of equal depth. (A batch is 24 pixels wide:
    single precision, and lod_percent 50 and 10 draw the first 32 and 19 points of every chain.)"""
    return _camera(name, 16)
