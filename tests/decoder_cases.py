"""Streams built to drive the decode loops into stated states, and the arithmetic that proves which states they reach
(tests/test_decoder_cpu.py asserts every claim below on the CPU, from the oracle's lane words and tables; tests/test_gpu_decoder.py
holds k_render, k_decode_points and the decode_chain() calls against the oracle on them). Inputs and integer arithmetic only.

Every stream is encoded unsorted: chain c of a batch is rows 64 c .. 64 c + 63 as given, its first delta the stored 0, so a stream is
written down as deltas [1024, 64, 3] per batch and the rows are their running sums. A batch's alphabet is what its deltas make it.

  phases    one batch; code lengths 1 .. 12 and an escape key in one table (a comb: Fibonacci-like frequencies); every length and the
            escape as first, second and third symbol of a point; at every start offset 0 .. 31 a 3-bit point, a 36-bit point and a
            point for every number of retired words that offset admits; points of more than 32 bits in rows 1, 62 and 63
  runs      one batch; all 16 (escapes of the previous point, escapes of this point) pairs, all 8 escape patterns of a point wave
            uniformly and with neighbouring lanes differing, one chain whose 189 free symbols all escape
  pool      six batches, each zero deltas plus E one-off deltas: escape words at 13248, 13312, 13313 of the whole batch, 5120 and 5121 of
            the first half, 5121 of the second half; the word that crosses a pool's end lies inside a point of three escapes
  limits    five batches: the table values +-(2^21 - 1), +-2^21, +-(2^21 + 1) and 0 without an escape; the same with escapes; only
            the two values that fit the packed entry; those two and +2^21; those two and -2^21, the entry's sentinel (in the last two
            batches a single value decides the flag: one comparison off by one in table_value_fits unflags exactly one of them)
  lengths   three batches: identical points (the single-symbol alphabet: 8 words a chain); whole waves of 8-word chains alternating
            with whole waves of chains of 72 words and more, ending on a long wave, and ending on a short one

`phases`, `runs` and `lengths` also exist as BC7 streams. What is impossible is not built, and tests/test_decoder_cpu.py says why
next to the assertion: row 0 of a chain is three codes of delta 0, which 3072 of a batch's 196 608 symbols are -- no clipped Huffman
code gives it more than 8 bits, so row 0 never has more than 32; and a point of b in 3 .. 36 bits at offset o retires (o + b) // 32
words, so two words retire only from offsets 28 .. 31 and none only up to offset 28."""
from __future__ import annotations

import ctypes as C
import functools
import os
import re

import numpy as np

import pcrhpg24_amd as P
from pcrhpg24_amd import build
from tests import oracle
from tests import select_cases as S

PPB = S.PPB
CHAINS, ROWS, SYMBOLS = 1024, 64, 192               # chains of a batch, points of a chain, symbols of a chain
TABLE = 4096
MAX_LEN = 12
STREAMS = ("phases", "runs", "pool", "limits", "lengths")
BC7_STREAMS = ("phases", "runs", "lengths")

# ---- constants of csrc/pcr_kernels.hip.h, restated; tests/test_decoder_cpu.py pins them to the source text ------------------------
ESC_POOL_WORDS = 13312
ESC_POOL_WORDS_HALF = 5120
ESC_SLACK = 64
TE_SLOW_VALUE = -(1 << 21)
TE_VALUE_SHIFT = 10
PINNED = {
    "ESC_POOL_WORDS": r"constexpr int ESC_POOL_WORDS = (\d+);",
    "ESC_POOL_WORDS_HALF": r"constexpr int ESC_POOL_WORDS_HALF\s+= (\d+);",
    "ESC_SLACK": r"constexpr int ESC_SLACK\s+= (\d+);",
    "TE_SLOW_VALUE": r"constexpr int32_t TE_SLOW_VALUE = -\(1 << (\d+)\);",
    "TE_VALUE_SHIFT": r"constexpr int TE_VALUE_SHIFT = (\d+);",
}
# the rule itself, as k_transcode and its helpers spell it
RULE_TEXT = (
    "return min(esc_count + (uint32_t)ESC_SLACK, (uint32_t)esc_pool_max(parts));",
    "return parts == 1 ? ESC_POOL_WORDS : ESC_POOL_WORDS_HALF;",
    "const bool over1 = nesc && sp0 + nesc > esc_pool_words(esc_total, 1);",
    "const bool over2 = nesc && (sp0 - e0) + nesc > esc_pool_words(e1 - e0, 2);",
    "const uint32_t e0 = tid < 512u ? 0u : esc_mid, e1 = tid < 512u ? esc_mid : esc_total;",
    "return value > TE_SLOW_VALUE && value < -TE_SLOW_VALUE;",
    "if (len > 0 && !table_value_fits(value)) generic = true;",
)


def kernel_source() -> str:
    return open(os.path.join(build.CSRC, "pcr_kernels.hip.h")).read()


def source_constants(text: str) -> dict:
    """The pinned constants as the kernel source has them (TE_SLOW_VALUE from its shift)."""
    out = {k: int(re.search(rx, text).group(1)) for k, rx in PINNED.items()}
    out["TE_SLOW_VALUE"] = -(1 << out["TE_SLOW_VALUE"])
    return out


# ---- the oracle's arrays of one batch ---------------------------------------------------------------------------------------------
def _i32(ptr, n):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_int32)), (n,))


def table_of(of, b):
    """(dt_cwlen, dt_values) of batch b, int32 [4096] each: length > 0 in the table, <= 0 an escape of -length bits."""
    nb = of.num_batches
    return _i32(of.s.dt_cwlen, nb * TABLE)[b * TABLE:(b + 1) * TABLE], _i32(of.s.dt_values, nb * TABLE)[b * TABLE:(b + 1) * TABLE]


def separate_sizes(of, b):
    """The inclusive prefix of the escape words the encoder wrote per chain, int64 [1024]."""
    return _i32(of.s.separate_sizes, of.num_batches * CHAINS)[b * CHAINS:(b + 1) * CHAINS].astype(np.int64)


def start_values(of, b):
    return _i32(of.s.start_values, of.num_batches * CHAINS * 3)[b * CHAINS * 3:(b + 1) * CHAINS * 3].reshape(CHAINS, 3)


# ---- the walk ---------------------------------------------------------------------------------------------------------------------
def walk(of, b) -> dict:
    """One batch's decode restated in numpy from of.lane_words(b) and the batch's table, all 1024 chains at once, 192 steps: a
    chain's bit stream is its own words in order, a symbol's key the 12 bits at its position. Per chain and symbol [1024, 192]:
      length, escape, value (the table's value under the key, whatever `escape` says), bitpos (in the chain's own stream)
    per chain and point [1024, 64]:
      offset (the point's first bit mod 32), bits (3 .. 36), retired = (offset + bits) // 32 (words the point finishes), n_escapes
    per chain [1024]:
      esc_words   escapes over all 192 symbols, symbols decoded from tail garbage included: k_transcode's `nesc`
      first_esc   the chain's first word in the batch's escape stream: k_transcode's `sp0`
      words       2 + (all bits) // 32: what the lockstep walk hands the chain
    and `delta` [1024, 192] (int32: the table value or the escape word read, over-reads behind the batch's own words included) and
    `xyz` [1024, 64, 3], the points those deltas give from the start values with int32 wrap-around."""
    words, counts = of.lane_words(b)
    cwlen, values = table_of(of, b)
    w = np.concatenate([words.T.astype(np.uint64), np.zeros((CHAINS, 4), np.uint64)], axis=1)       # [1024, 84]
    rows = np.arange(CHAINS)
    pos = np.zeros(CHAINS, np.int64)
    length, escape, value, bitpos = (np.zeros((CHAINS, SYMBOLS), t) for t in (np.int64, bool, np.int32, np.int64))
    for k in range(SYMBOLS):
        r, o = pos >> 5, (pos & 31).astype(np.uint64)
        two = (w[rows, r] << np.uint64(32)) | w[rows, r + 1]
        key = ((two >> (np.uint64(52) - o)) & np.uint64(0xFFF)).astype(np.int64)
        bitpos[:, k] = pos
        length[:, k] = np.abs(cwlen[key])
        escape[:, k] = cwlen[key] <= 0
        value[:, k] = values[key]
        pos = pos + length[:, k]
    bits = length.reshape(CHAINS, ROWS, 3).sum(axis=2)
    offset = bitpos[:, ::3] & 31
    esc_words = escape.sum(axis=1).astype(np.int64)
    ssz = separate_sizes(of, b)
    first_esc = np.concatenate([[0], ssz[:-1]])
    # the escape word of every escaping symbol: the chain's next one, from the whole stream's array (a garbage tail may read on)
    sep = of.separate()
    base = int(of.batch(b).separate_batch_offset)
    nth = np.cumsum(escape, axis=1) - escape                        # escapes of the chain before this symbol
    at = np.minimum(base + first_esc[:, None] + nth, len(sep) - 1)
    delta = np.where(escape, sep[at], value).astype(np.int32)
    steps = delta.reshape(CHAINS, ROWS, 3).astype(np.int64)
    xyz = (start_values(of, b).astype(np.int64)[:, None, :] + np.cumsum(steps, axis=1))
    xyz = ((xyz + (1 << 31)) % (1 << 32) - (1 << 31)).astype(np.int32)
    return dict(length=length, escape=escape, value=value, bitpos=bitpos, offset=offset, bits=bits, retired=(offset + bits) >> 5,
                n_escapes=escape.reshape(CHAINS, ROWS, 3).sum(axis=2), esc_words=esc_words, first_esc=first_esc,
                words=2 + (pos >> 5), lane_counts=counts.astype(np.int64), delta=delta, xyz=xyz, separate_sizes=ssz)


def value_fits(v) -> np.ndarray:
    """table_value_fits of csrc/pcr_kernels.hip.h: strictly between -2^21 and 2^21 (-2^21 itself is the entry's sentinel)."""
    v = np.asarray(v, np.int64)
    return (v > TE_SLOW_VALUE) & (v < -TE_SLOW_VALUE)


def pool_words(esc_count, parts: int):
    """esc_pool_words: the escape words k_render keeps in LDS for a workgroup whose own chains have esc_count."""
    return np.minimum(np.asarray(esc_count, np.int64) + ESC_SLACK, ESC_POOL_WORDS if parts == 1 else ESC_POOL_WORDS_HALF)


def expected_flags(of, b, w=None) -> tuple[int, int]:
    """(BF_GENERIC_SLOW_PATH, BF_GENERIC_SLOW_PATH_HALF) of batch b as k_transcode sets them: a wide in-table value sets both; else
    a chain that reads an escape word behind the pool of its workgroup -- the whole batch's pool, or its half's -- sets that one."""
    w = walk(of, b) if w is None else w
    cwlen, values = table_of(of, b)
    generic = bool(((cwlen > 0) & ~value_fits(values)).any())
    nesc, sp0, ssz = w["esc_words"], w["first_esc"], w["separate_sizes"]
    esc_total, esc_mid = int(ssz[1023]), int(ssz[511])
    over1 = (nesc > 0) & (sp0 + nesc > pool_words(esc_total, 1))
    tid = np.arange(CHAINS)
    e0, e1 = np.where(tid < 512, 0, esc_mid), np.where(tid < 512, esc_mid, esc_total)
    over2 = (nesc > 0) & ((sp0 - e0) + nesc > pool_words(e1 - e0, 2))
    return int(generic or over1.any()), int(generic or over2.any())


# ---- from deltas to a stream ------------------------------------------------------------------------------------------------------
def rows_of(deltas, start):
    """int64 [65536, 3]: the running sums of deltas [1024, 64, 3] (row 0 of every chain is 0) from start [1024, 3]."""
    d = np.asarray(deltas, np.int64)
    assert d.shape == (CHAINS, ROWS, 3) and not d[:, 0].any()
    return (np.asarray(start, np.int64)[:, None, :] + np.cumsum(d, axis=1)).reshape(PPB, 3)


def grid_start(spacing=4096, base=(0, 0, 0)):
    """Chain c starts at column c % 32, row c // 32 of a grid on z = 0."""
    c = np.arange(CHAINS)
    return np.stack([c % 32 * spacing, c // 32 * spacing, np.zeros(CHAINS, np.int64)], axis=1) + np.asarray(base, np.int64)


def encode(batches, pad_tails: bool, bc7: bool = False):
    """The .huffman image of the batches (each int64 [65536, 3], rows in the order given)."""
    xyz = np.concatenate(batches)
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    assert lo.min() > -(1 << 31) and hi.max() < (1 << 31)
    c = np.random.default_rng(12).integers(0, 1 << 24, len(xyz)).astype(np.uint32)
    x, y, z = (np.ascontiguousarray(xyz[:, k].astype(np.int32)) for k in range(3))
    las = S.las_for(tuple(int(v) for v in lo), tuple(int(v) + 1 for v in hi))
    image, st = P.encode_points(x, y, z, c, las, morton_sort=False, nthreads=2, pad_tails=pad_tails, bc7=bc7)
    assert st["num_batches"] == len(batches)
    return S._keep(image)


class OneOffs:
    """Distinct deltas that occur once each in a batch, so that the clipped code escapes them: +m, -m, +(m + 1), -(m + 1), ... --
    a + and its - follow each other, which keeps the coordinates of a chain bounded."""

    def __init__(self, first: int):
        self.j, self.first = 0, first

    def __call__(self) -> int:
        v = (self.first + self.j // 2) * (1 if self.j % 2 == 0 else -1)
        self.j += 1
        return v


# ---- phases -----------------------------------------------------------------------------------------------------------------------
ESC = 13                                            # the class "escape" beside the classes 1 .. 12 (= the code length)
PHASES_ONE_OFFS = 400
PHASES_VALUE = {k: (k // 2) * (1 if k % 2 == 0 else -1) for k in range(2, MAX_LEN + 1)}     # class -> delta: +1, -1, +2, -2, ..., +6
PHASES_VALUE[1] = 0
SPECIALS = ((ESC, ESC, ESC), (12, 12, 12), (10, 10, 10))                                     # 36, 36 and 30 bits


def comb_counts(one_offs: int) -> dict:
    """Frequencies under which the Huffman tree is a comb -- one leaf at every depth 1 .. 12 and the subtree of the one-off deltas
    beside the leaf at depth 12: class k has to outweigh class k + 1 and everything below it (a Fibonacci-like growth, every
    comparison strict so that no tie decides the shape). Class 1, delta 0, takes what is left of the batch's 196 608 symbols."""
    count = {12: one_offs + 1}
    under = one_offs                                # weight of the subtree beside the leaf of class k
    for k in range(MAX_LEN, 1, -1):
        nxt = max(count[k], under) + 1
        under += count[k]
        count[k - 1] = nxt
    under += count[1]
    count[1] += 3 * PPB - under
    assert count[1] > count[2] and sum(count.values()) + one_offs == 3 * PPB
    return count


def row_at_offset(o: int) -> int:
    """The row of an otherwise all-zero chain (3 bits a point) that starts at bit offset o mod 32: 3 j = o, 1 <= j <= 32."""
    j = 11 * o % 32                                 # 3 * 11 = 33 = 1 (mod 32)
    return j if j else 32


@functools.lru_cache(maxsize=None)
def phases_plan():
    """classes int64 [1024, 64, 3] (1 .. 12: the code length wanted, 13: an escape) of `phases`, and what lies where:
      chains 0 .. 95    3 o + t: all-zero chains (3 bits a point, so row j starts at offset 3 j mod 32) with SPECIALS[t] at the row
                        that starts at offset o
      chains 96 .. 99   36-bit points (three escapes; three codes of 12) at rows 62 and 63
      chain 100         rows 1 .. 13: (class r, class r + 1, class r + 2), cyclically over the 13 classes
      the rest          what is left of the comb's frequencies, dealt out with a fixed stride"""
    cls = np.zeros((CHAINS, ROWS, 3), np.int64)
    cls[:, 0] = 1
    free = np.ones((CHAINS, ROWS), bool)
    free[:, 0] = False
    for o in range(32):
        for t, special in enumerate(SPECIALS):
            c = 3 * o + t
            cls[c, 1:] = 1
            cls[c, row_at_offset(o)] = special
            free[c] = False
    for c, (row, special) in enumerate(((62, SPECIALS[0]), (63, SPECIALS[0]), (62, SPECIALS[1]), (63, SPECIALS[1])), start=96):
        cls[c, 1:] = 1
        cls[c, row] = special
        free[c] = False
    order = list(range(1, 14))
    for r in range(1, 14):
        cls[100, r] = [order[(r - 1 + k) % 13] for k in range(3)]
        free[100, r] = False
    want = dict(comb_counts(PHASES_ONE_OFFS))
    want[ESC] = PHASES_ONE_OFFS
    used = np.bincount(cls[~free].reshape(-1), minlength=14)
    left = np.concatenate([np.full(want[k] - used[k], k) for k in range(1, 14)])
    slots = int(free.sum()) * 3
    assert len(left) == slots and all(want[k] >= used[k] for k in want)
    stride = 121_501                                # odd and no multiple of 3 or of the other factors checked below
    assert np.gcd(stride, slots) == 1
    cls[free] = left[np.arange(slots, dtype=np.int64) * stride % slots].reshape(-1, 3)
    cls.setflags(write=False)
    return cls


def phases_points():
    cls = phases_plan()
    one_off = OneOffs(100)
    d = np.zeros((CHAINS, ROWS, 3), np.int64)
    for k, v in PHASES_VALUE.items():
        d[cls == k] = v
    where = np.nonzero(cls == ESC)
    d[where] = [one_off() for _ in range(len(where[0]))]
    return [rows_of(d, grid_start())]


# ---- runs -------------------------------------------------------------------------------------------------------------------------
TRANSITIONS = (0, 0, 1, 0, 2, 0, 3, 1, 1, 2, 1, 3, 2, 2, 3, 3, 0)      # every ordered pair of 0 .. 3 once: a de Bruijn cycle, closed
RUNS_ALL_ESCAPING = 200                             # the chain whose 189 free symbols escape


@functools.lru_cache(maxsize=None)
def runs_plan():
    """escape bool [1024, 64, 3] of `runs` (everything else is delta 0):
      wave 0          row r = 1 .. 8: pattern r - 1 (bit k: symbol k escapes) in all 64 chains
      wave 1          row r = 1 .. 8: pattern (lane + r - 1) % 8 -- neighbouring lanes differ at every row
      wave 2          rows 0 .. 16: TRANSITIONS[r] escapes; which symbols they are depends on the lane
      chain 200       rows 1 .. 63 escape whole
      chains 512 ..   two points of three escapes (rows 1 and 2), so that the batch has more than 4096 one-off deltas
    Either half stays under its pool: the batch is unflagged and k_render reads every escape unchecked."""
    e = np.zeros((CHAINS, ROWS, 3), bool)
    bits = lambda p: [bool(p >> k & 1) for k in range(3)]
    for lane in range(64):
        for r in range(1, 9):
            e[lane, r] = bits(r - 1)
            e[64 + lane, r] = bits((lane + r - 1) % 8)
        for r, n in enumerate(TRANSITIONS):
            e[128 + lane, r] = {0: [0, 0, 0], 1: [k == lane % 3 for k in range(3)], 2: [k != lane % 3 for k in range(3)], 3: [1, 1, 1]}[n]
    e[RUNS_ALL_ESCAPING, 1:] = True
    e[512:, 1:3] = True
    assert not e[:, 0].any()
    e.setflags(write=False)
    return e


def runs_points():
    e = runs_plan()
    one_off = OneOffs(1)
    d = np.zeros((CHAINS, ROWS, 3), np.int64)
    where = np.nonzero(e)
    d[where] = [one_off() for _ in range(len(where[0]))]
    return [rows_of(d, grid_start(1 << 15))]


# ---- pool -------------------------------------------------------------------------------------------------------------------------
# (escape words of chains 0 .. 511, of chains 512 .. 1023) of the six batches
POOL_HALVES = ((6624, 6624), (6656, 6656), (6656, 6657), (5120, 300), (5121, 300), (300, 5121))
POOL_TOTALS = tuple(a + b for a, b in POOL_HALVES)
# the first flag is the claim; the second one follows by arithmetic (a half of more than 5120 words is over its pool, and no batch of
# more than 2 * 5120 words can have two halves that are not)
POOL_FLAGS = ((0, 1), (0, 1), (1, 1), (0, 0), (0, 1), (0, 1))


def pool_half(count: int, one_off):
    """deltas [512, 64, 3]: `count` one-off deltas as points of three, dealt evenly from row 1 on, the later chains one point more;
    what does not fill a point of three comes first, in row 1 of the half's first chain. So the half's last escape words belong
    to a point of three escapes of its last chain."""
    d = np.zeros((512, ROWS, 3), np.int64)
    points, rest = divmod(count, 3)
    for c in range(512):
        row = 1
        if c == 0 and rest:
            d[c, row, :rest] = [one_off() for _ in range(rest)]
            row += 1
        for _ in range(points // 512 + (c >= 512 - points % 512)):
            d[c, row] = [one_off() for _ in range(3)]
            row += 1
    return d


def pool_points():
    out = []
    for first, second in POOL_HALVES:
        one_off = OneOffs(1)
        out.append(rows_of(np.concatenate([pool_half(first, one_off), pool_half(second, one_off)]), grid_start(1 << 15)))
    return out


# ---- limits -----------------------------------------------------------------------------------------------------------------------
LIMIT = 1 << 21
LIMIT_VALUES = (LIMIT - 1, -(LIMIT - 1), LIMIT, -LIMIT, LIMIT + 1, -(LIMIT + 1))    # a + and its - follow each other
LIMITS_ONE_OFFS = 300
LIMITS_FLAGS = ((1, 1), (1, 1), (0, 0), (1, 1), (1, 1))


def limits_points():
    """Batch 0: row r, axis k of every chain steps by LIMIT_VALUES[(r - 1 + 2 k) % 6]: seven symbols with the stored 0, no escape.
    Batch 1: the same, with 300 one-off deltas in rows 1 .. 5 of chains 0 .. 19 (all three symbols). Batch 2: +-(2^21 - 1) only.
    Batches 3 and 4: the cycle (v, -(2^21 - 1), 2^21 - 1, -(2^21 - 1)) with v = 2^21 and the cycle negated with v = -2^21: the one
    value that does not fit occurs at most 48 times a chain -- fewer than the ESC_SLACK words every pool has, which is all a kernel
    could read if it took the batch for unflagged and the sentinel entry for an escape."""
    r, k = np.meshgrid(np.arange(ROWS), np.arange(3), indexing="ij")
    cycle = np.array(LIMIT_VALUES, np.int64)
    wide = np.broadcast_to(cycle[(r - 1 + 2 * k) % 6], (CHAINS, ROWS, 3)).copy()
    wide[:, 0] = 0
    with_escapes = wide.copy()
    one_off = OneOffs(1000)
    for c in range(LIMITS_ONE_OFFS // 15):
        for row in range(1, 6):
            with_escapes[c, row] = [one_off() for _ in range(3)]
    fits = np.broadcast_to(cycle[(r - 1 + k) % 2], (CHAINS, ROWS, 3)).copy()
    fits[:, 0] = 0
    single = np.array([LIMIT, -(LIMIT - 1), LIMIT - 1, -(LIMIT - 1)], np.int64)
    upper = np.broadcast_to(single[(r - 1 + k) % 4], (CHAINS, ROWS, 3)).copy()
    upper[:, 0] = 0
    start = grid_start(1 << 15, (1 << 23, 1 << 23, 1 << 23))
    return [rows_of(d, start) for d in (wide, with_escapes, fits, upper, -upper)]


# ---- lengths ----------------------------------------------------------------------------------------------------------------------
SHORT_WORDS = 2 + SYMBOLS // 32                     # 8: every symbol one bit
LONG_WORDS = 2 + (63 * 36) // 32                    # 72: 63 points of 36 bits (and the stored 0)


def lengths_points():
    """Batch 0: 65 536 times one point. Batches 1 and 2: waves (64 chains) whose deltas are all 0 alternate with waves whose 189 free
    symbols are all one-off deltas; batch 1 begins with a zero wave and ends on a long one, batch 2 the other way round."""
    out = [np.tile(np.array([[7, -3, 11]], np.int64), (PPB, 1))]
    for first_long in (1, 0):
        one_off = OneOffs(1)
        d = np.zeros((CHAINS, ROWS, 3), np.int64)
        for wave in range(CHAINS // 64):
            if wave % 2 == first_long:
                d[64 * wave:64 * wave + 64, 1:] = np.array([one_off() for _ in range(64 * 189)], np.int64).reshape(64, 63, 3)
        out.append(rows_of(d, grid_start(1 << 17)))
    return out


def long_waves(b: int):
    """The waves of batch b of `lengths` whose chains are long (none in batch 0)."""
    return [] if b == 0 else [w for w in range(CHAINS // 64) if w % 2 == (1 if b == 1 else 0)]


# ---- the streams ------------------------------------------------------------------------------------------------------------------
BUILDERS = {"phases": phases_points, "runs": runs_points, "pool": pool_points, "limits": limits_points, "lengths": lengths_points}
VARIANTS = [(name, pad, False) for name in STREAMS for pad in (True, False)] + [(name, True, True) for name in BC7_STREAMS]


def variant_id(v) -> str:
    return f"{v[0]}-{'padded' if v[1] else 'plain'}{'-bc7' if v[2] else ''}"


@functools.lru_cache(maxsize=None)
def points(name: str):
    """The rows of a stream as given to the encoder: a tuple of int64 [65536, 3] (read-only), one per batch."""
    out = tuple(np.ascontiguousarray(p, np.int64) for p in BUILDERS[name]())
    for p in out:
        p.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def stream(name: str, pad_tails: bool = True, bc7: bool = False):
    return encode(points(name), pad_tails, bc7)


@functools.lru_cache(maxsize=None)
def oracle_file(name: str, pad_tails: bool = True, bc7: bool = False) -> oracle.OracleFile:
    return oracle.OracleFile(stream(name, pad_tails, bc7))


@functools.lru_cache(maxsize=None)
def walks(name: str, pad_tails: bool = True, bc7: bool = False):
    of = oracle_file(name, pad_tails, bc7)
    return tuple(walk(of, b) for b in range(of.num_batches))


# ---- what the flags are made of -----------------------------------------------------------------------------------------------------
def has_wide_value(of, b) -> bool:
    cwlen, values = table_of(of, b)
    return bool(((cwlen > 0) & ~value_fits(values)).any())


def escape_index(w):
    """int64 [1024, 192]: the index in the batch's escape stream of the word every escaping symbol reads (-1 elsewhere)."""
    nth = np.cumsum(w["escape"], axis=1) - w["escape"]
    return np.where(w["escape"], w["first_esc"][:, None] + nth, -1)


def crossing(w, part: int):
    """The symbol that reads the first word behind the pool of the whole batch (part None), or of the half `part`, as (chain, symbol,
    escapes of its point, escapes of its point before it); None if no symbol does."""
    ssz = w["separate_sizes"]
    e0, count = (0, int(ssz[1023])) if part is None else ((0, int(ssz[511])) if part == 0 else (int(ssz[511]), int(ssz[1023] - ssz[511])))
    limit = e0 + int(pool_words(count, 1 if part is None else 2))
    idx = escape_index(w)
    if part is not None:
        idx = np.where((np.arange(CHAINS) // 512 == part)[:, None], idx, -1)
    at = np.argwhere(idx == limit)
    if not len(at):
        return None
    c, k = (int(v) for v in at[0])
    point = w["escape"][c, k - k % 3:k - k % 3 + 3]
    return c, k, int(point.sum()), int(point[:k % 3].sum())


# ---- cameras ----------------------------------------------------------------------------------------------------------------------
WIDTH, HEIGHT = 320, 200
FAR_FACTOR, FAR_LOD = 40.0, 20                      # the far camera: so many times the near one's distance, at this lod_percent


def cameras(name: str):
    """(near, far): a camera straight above the middle of the stream's box that sees all of it (lod_percent 100, no culling: every
    point is walked), and one FAR_FACTOR times as high with lod_percent FAR_LOD, under which every batch is drawn with npr < 64."""
    from tests import scenes
    xyz = np.concatenate(points(name))
    span = (xyz.max(axis=0) - xyz.min(axis=0) + 1) * 0.001          # the renderers see (lattice - min) * scale
    target = tuple(float(v) / 2 for v in span)
    radius = 1.5 * float(max(span[0] * HEIGHT / WIDTH, span[1], 1.0)) + float(span[2])
    near = scenes.straight_down(radius, target, WIDTH, HEIGHT, far=1000.0 * radius)
    far = scenes.with_flags(scenes.straight_down(FAR_FACTOR * radius, target, WIDTH, HEIGHT, far=1000.0 * radius), lod_percent=FAR_LOD, cull=1)
    return near, far


def stream_by_id(vid: str):
    """The image of the variant that variant_id() names."""
    return stream(*{variant_id(v): v for v in VARIANTS}[vid])
