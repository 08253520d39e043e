"""Inputs built so that the GPU encoder's own rules decide -- the stable Morton sort, the tie rules of the Huffman construction, the
owner of a shared escape key, the word edges of packing and interleaving, chunk edges, the colour blocks -- with the numpy
restatements that prove what each input is (tests/test_encoder_cases_cpu.py asserts every claim below with the CPU encoder and the
oracle; tests/test_gpu_encoder_cases.py holds Context.gpu_encode_points byte for byte against the CPU encoder on them). Inputs and
integer arithmetic only; nothing here is taken from a GPU.

Every builder returns (x, y, z, colour, las, kwargs): int32 / uint32 arrays from fixed seeds and the keyword arguments both encoders
get. The unsorted ones are written down as deltas [1024, 64, 3] as in tests/decoder_cases.py (chain c is rows 64 c .. 64 c + 63).

  key_ties      sorted, 2 x 65536 + 1000 points whose shifted coordinates have bits 0, 1, 21, 22, 30 and 31 only: 2^17 possible keys
                for 132 072 points, keys that differ only in `hi`, only in bit 63 of `lo`, only in bits 0 / 1 of `hi` -- and pairs
                that differ in X bit 31, which morton_key drops: equal keys, other points. Distinct colours, so a tie broken the
                other way moves a colour block as well
  two_symbols   x += 5 along every chain: the alphabet {0, 5}, one bit each, 192 bits = 6 whole words a chain, no partial word
  fib, pow2     x deltas +1, -1, +2, -2, ... with the frequencies 1, 1, 2, 3, 5, ... (22 terms) and 1, 1, 2, 4, ..., 16384: the
                tree is deeper than 12 and its rarest leaves escape under one shared 12-bit key; in `pow2` every merge but the first
                ties a leaf with an internal node, in `fib` only the second does (the sums are one short of the next leaf)
  flat          8064 distinct x deltas 8 times each (all escape), 64 y deltas 32 times each (they tie with internal nodes and escape)
                and 64 y deltas 40 times each (12 bits in the table): equal frequencies throughout, the order of the leaves is the
                stable frequency sort's alone, and 1984 escape keys have several owners to choose from
  mixed_lanes   even lanes of every cluster all-zero chains, odd lanes 189 one-off deltas: the shortest chain beside the longest
  colours       constructed colour blocks: the reference encoder's 256, greys, solid, two-colour, ramps, black / white, and blocks
                that repeat earlier ones with the top byte set
  n1, n65536, n65537, chunks3, key_ties_chunks
                sorted shapes on key_ties' generator: one point, a whole batch, a batch and one point, three whole chunks of a batch,
                chunks sorted one by one with a last chunk of 1000 points
  dec_<name>    the five streams of tests/decoder_cases.py as points, with its colours and LAS header"""
from __future__ import annotations

import functools
import os

import numpy as np

import pcrhpg24_amd as P
from tests import select_cases as S
from tests.decoder_cases import CHAINS, ROWS, STREAMS, TABLE, OneOffs, grid_start, rows_of, table_of  # noqa: F401  (table_of: for the CPU test)
from tests.decoder_cases import points as decoder_points
from tests.decoder_cases import stream as decoder_stream  # noqa: F401  (the image a dec_<name> case has to become)

PPB = S.PPB
CLUSTERS, LANES = 32, 32                            # clusters of a batch, chains of a cluster
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CHUNK = 4 * PPB                                     # scratch for four batches; with n <= 4 batches the image does not depend on it
DECODER_CHUNK = 8 * PPB                             # `pool` has six batches: one chunk, as under the default of 100 batches

# ---- figures: stated by the issue where it measured them, else taken from the CPU encoder (tests/test_encoder_cases_cpu.py) --------
KEY_TIES_N = 2 * PPB + 1000
KEY_TIES = dict(distinct_keys=83_210, points_sharing_a_key=83_830, points_in_groups_that_differ_in_x=52_741, distinct_hi=1024,
                distinct_lo=128, rows_moved_by_descending_ties=38_078)
TWO_SYMBOLS = dict(encoded_plain=24_576, encoded_padded=32_768, escaped=0)
FIB_TERMS, FIB_SYMBOLS, FIB_ESCAPED = 22, 46_367, 232
POW2_TERMS, POW2_SYMBOLS = 16, 32_768
POW2_ESCAPED = 16                                   # CPU encoder: the five rarest symbols, 1 + 1 + 2 + 4 + 8
FLAT_ESCAPED = 66_560                               # CPU encoder: all 8064 x 8 x deltas and the 64 x 32 tied y deltas
FLAT_ESCAPE_KEYS = 1984                             # CPU encoder: 12-bit keys that 8128 escaping symbols share
MIXED_ESCAPED = 96_768                              # CPU encoder: all 512 x 189 one-off deltas
MIXED_BITS = (192, 3 + 189 * 12)                    # CPU encoder's table: 1 bit for delta 0, 12 for an escape: 6 and 71 words


# ---- the Morton key, restated -----------------------------------------------------------------------------------------------------
def shifted(v) -> np.ndarray:
    """shift_coord: the coordinate as an unsigned number, v + 2^31."""
    return (np.asarray(v, np.int64) + (1 << 31)).astype(np.uint64)


def spread(v) -> np.ndarray:
    """Bits 0 .. 20 of v at positions 3 i."""
    v = np.asarray(v, np.uint64)
    out = np.zeros(v.shape, np.uint64)
    for i in range(21):
        out |= ((v >> np.uint64(i)) & np.uint64(1)) << np.uint64(3 * i)
    return out


def key(x, y, z):
    """(hi, lo) of morton_key on the shifted coordinates: lo = the three 21-bit spreads and X bit 21 at bit 63; hi = Y bit 21 at bit
    0, Z bit 21 at bit 1 and, for i = 22 .. 31, X at 3 (i - 21) + 2, Y at 3 (i - 21), Z at 3 (i - 21) + 1 -- cut to 32 bits, which
    drops X bit 31 (it would be bit 32)."""
    X, Y, Z = shifted(x), shifted(y), shifted(z)
    one = np.uint64(1)
    bit = lambda v, i: (v >> np.uint64(i)) & one
    lo = spread(X) | spread(Y) << one | spread(Z) << np.uint64(2) | bit(X, 21) << np.uint64(63)
    hi = bit(Y, 21) | bit(Z, 21) << one
    for i in range(22, 32):
        hi |= bit(X, i) << np.uint64(3 * (i - 21) + 2) | bit(Y, i) << np.uint64(3 * (i - 21)) | bit(Z, i) << np.uint64(3 * (i - 21) + 1)
    return hi & np.uint64(0xFFFFFFFF), lo


def sorted_order(x, y, z, descending_ties: bool = False) -> np.ndarray:
    """The permutation of a stable sort by (hi, lo): ties in input order, or -- the wrong way -- in reverse."""
    hi, lo = key(x, y, z)
    idx = np.arange(len(hi), dtype=np.int64)
    return np.lexsort((-idx if descending_ties else idx, lo, hi))


def padded(arrays, n_to: int):
    """The arrays with their last element repeated up to n_to rows: what either encoder does to a ragged chunk before it sorts."""
    return tuple(np.concatenate([a, np.full(n_to - len(a), a[-1], a.dtype)]) for a in arrays)


# ---- sorted inputs ----------------------------------------------------------------------------------------------------------------
def tie_points(n: int):
    """One default_rng(5); for each of x, y, z in that order: the low two bits, then bits 21, 22, 30 and 31 of the shifted coordinate."""
    rng = np.random.default_rng(5)
    out = []
    for _ in range(3):
        v = rng.integers(0, 4, n)
        for b in (21, 22, 30, 31):
            v = v | rng.integers(0, 2, n) << b
        out.append((v - (1 << 31)).astype(np.int32))
    colour = (np.arange(n, dtype=np.int64) & 0xFFFFFF).astype(np.uint32)
    las = S.las_for((-(1 << 31),) * 3, (1 << 31,) * 3)
    return out[0], out[1], out[2], colour, las


def _sorted_case(n: int, chunk_points: int = CHUNK):
    return (*tie_points(n), dict(morton_sort=True, chunk_points=chunk_points))


# ---- unsorted inputs --------------------------------------------------------------------------------------------------------------
def _unsorted_case(deltas, start, colour=None, chunk_points: int = CHUNK):
    xyz = rows_of(deltas, start)
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    assert lo.min() > -(1 << 31) and hi.max() < (1 << 31)
    if colour is None:
        colour = np.random.default_rng(12).integers(0, 1 << 24, len(xyz)).astype(np.uint32)
    x, y, z = (np.ascontiguousarray(xyz[:, k].astype(np.int32)) for k in range(3))
    las = S.las_for(tuple(int(v) for v in lo), tuple(int(v) + 1 for v in hi))
    return x, y, z, colour, las, dict(morton_sort=False, chunk_points=chunk_points)


def two_symbols_deltas():
    d = np.zeros((CHAINS, ROWS, 3), np.int64)
    d[:, 1:, 0] = 5
    return d


def signed_values(terms: int) -> np.ndarray:
    """+1, -1, +2, -2, ...: term k is (k // 2 + 1) with the sign of (-1)^k."""
    k = np.arange(terms)
    return (k // 2 + 1) * np.where(k % 2 == 0, 1, -1)


def fib_frequencies() -> np.ndarray:
    f = [1, 1]
    while len(f) < FIB_TERMS:
        f.append(f[-1] + f[-2])
    return np.array(f, np.int64)


def pow2_frequencies() -> np.ndarray:
    return np.array([1] + [1 << k for k in range(POW2_TERMS - 1)], np.int64)


def _frequency_deltas(freqs):
    """The 63 x 1024 free x symbols: value k of signed_values freqs[k] times, the rest 0, shuffled with default_rng(1)."""
    free = np.zeros(CHAINS * (ROWS - 1), np.int64)
    body = np.repeat(signed_values(len(freqs)), freqs)
    free[:len(body)] = body
    np.random.default_rng(1).shuffle(free)
    d = np.zeros((CHAINS, ROWS, 3), np.int64)
    d[:, 1:, 0] = free.reshape(CHAINS, ROWS - 1)
    return d


def batch_frequencies(freqs) -> dict:
    """symbol -> frequency of the whole batch of _frequency_deltas(freqs): delta 0 takes every other symbol of the 196 608."""
    out = {int(v): int(f) for v, f in zip(signed_values(len(freqs)), freqs)}
    out[0] = 3 * PPB - int(np.sum(freqs))
    return out


FLAT_VALUES, FLAT_TIMES = 8064, 8
FLAT_TIED = (4033, 64, 32)                          # first magnitude, values, times: as often as four of the x deltas together
FLAT_IN_TABLE = (4100, 64, 40)


def flat_class(first: int, values: int, times: int) -> np.ndarray:
    """+first, -first, +(first + 1), ...: the `values` distinct deltas of a class, each of which occurs `times` times."""
    k = np.arange(values)
    return (first + k // 2) * np.where(k % 2 == 0, 1, -1)


def flat_deltas():
    """x: +1, -1, +2, -2, ..., +4032, -4032, eight times over, along the free x symbols (a + and its - follow each other). With
    delta 0 in every other place the 8064 equal leaves all lie deeper than 12 -- Kraft's sum of 8064 codes of 12 bits is 1.97 --
    and the table has the lengths 1 and -12 only. So that the clip has both sides, y carries two small classes of equal
    frequencies more: 64 deltas 32 times each, which tie with the internal nodes of four x deltas (and escape), and 64 deltas 40
    times each, which get 12 bits in the table."""
    d = np.zeros((CHAINS, ROWS, 3), np.int64)
    d[:, 1:, 0] = np.tile(signed_values(FLAT_VALUES), FLAT_TIMES).reshape(CHAINS, ROWS - 1)
    free = np.zeros(CHAINS * (ROWS - 1), np.int64)
    body = np.concatenate([np.tile(flat_class(*c), c[2]) for c in (FLAT_TIED, FLAT_IN_TABLE)])
    free[:len(body)] = body
    d[:, 1:, 1] = free.reshape(CHAINS, ROWS - 1)
    return d


def mixed_lanes_deltas():
    one_off = OneOffs(1)
    d = np.zeros((CHAINS, ROWS, 3), np.int64)
    for c in range(1, CHAINS, 2):
        d[c, 1:] = np.array([one_off() for _ in range(3 * (ROWS - 1))], np.int64).reshape(ROWS - 1, 3)
    return d


# ---- colours ----------------------------------------------------------------------------------------------------------------------
COLOUR_BLOCKS = PPB // 16
TWINS = 256                                         # blocks that repeat an earlier one with the top byte set
TWIN_FIRST = 256 * 4 + 3 * 64 + 256                 # the first of them: behind the reference's, grey, solid, two-colour, ramp, black / white


def twin_of(k) -> np.ndarray:
    """The earlier block that block TWIN_FIRST + k repeats: every 5th, which reaches all six kinds before it."""
    return (np.asarray(k) * 5 + 3) % TWIN_FIRST


def colour_blocks() -> np.ndarray:
    """uint32 [4096, 16], 0x00BBGGRR but for the twins' top byte."""
    rng = np.random.default_rng(31)
    px = np.arange(16, dtype=np.int64)
    parts = [np.load(os.path.join(G, "bc1_ref_blocks.npz"))["colors"].astype(np.int64)]
    parts.append(np.broadcast_to((np.arange(256, dtype=np.int64) * 0x010101)[:, None], (256, 16)))
    parts.append(np.broadcast_to(rng.integers(0, 1 << 24, 256)[:, None], (256, 16)))
    two = rng.integers(0, 1 << 24, (256, 2))
    parts.append(np.take_along_axis(two, rng.integers(0, 2, (256, 16)), axis=1))
    j = np.arange(64, dtype=np.int64)[:, None]
    ramp = np.minimum(255, 4 * j + px[None, :] * (j % 16 + 1))                  # from a flat step of 1 to one that saturates
    parts += [ramp << shift for shift in (0, 8, 16)]
    mask = rng.integers(0, 2, (256, 16))
    mask[0], mask[1] = 0, 1                                                     # all black, all white
    mask[2], mask[3] = px == 0, px != 15                                        # one pixel of the other kind
    parts.append(mask * 0xFFFFFF)
    early = np.concatenate(parts)
    assert len(early) == TWIN_FIRST
    parts.append(early[twin_of(np.arange(TWINS))] | 0xFF000000)
    parts.append(rng.integers(0, 1 << 24, (COLOUR_BLOCKS - TWIN_FIRST - TWINS, 16)))
    return np.concatenate(parts).astype(np.uint32)


# ---- the cases --------------------------------------------------------------------------------------------------------------------
def _decoder_case(name: str):
    xyz = np.concatenate(decoder_points(name))
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    colour = np.random.default_rng(12).integers(0, 1 << 24, len(xyz)).astype(np.uint32)          # decoder_cases.encode's
    x, y, z = (np.ascontiguousarray(xyz[:, k].astype(np.int32)) for k in range(3))
    las = S.las_for(tuple(int(v) for v in lo), tuple(int(v) + 1 for v in hi))
    return x, y, z, colour, las, dict(morton_sort=False, chunk_points=DECODER_CHUNK)


BUILDERS = {
    "key_ties": lambda: _sorted_case(KEY_TIES_N),
    "two_symbols": lambda: _unsorted_case(two_symbols_deltas(), grid_start(1 << 12)),
    "fib": lambda: _unsorted_case(_frequency_deltas(fib_frequencies()), grid_start(1 << 12, base=(1 << 20, 0, 0))),
    "pow2": lambda: _unsorted_case(_frequency_deltas(pow2_frequencies()), grid_start(1 << 12, base=(1 << 20, 0, 0))),
    "flat": lambda: _unsorted_case(flat_deltas(), grid_start(1 << 14, base=(1 << 20, 1 << 20, 0))),
    "mixed_lanes": lambda: _unsorted_case(mixed_lanes_deltas(), grid_start(1 << 17)),
    "colours": lambda: _unsorted_case(two_symbols_deltas(), grid_start(1 << 12), colour=colour_blocks().reshape(-1)),
    "n1": lambda: _sorted_case(1),
    "n65536": lambda: _sorted_case(PPB),
    "n65537": lambda: _sorted_case(PPB + 1),
    "chunks3": lambda: _sorted_case(3 * PPB, chunk_points=PPB),
    "key_ties_chunks": lambda: _sorted_case(KEY_TIES_N, chunk_points=PPB),
    **{f"dec_{name}": functools.partial(_decoder_case, name) for name in STREAMS},
}
CASES = tuple(BUILDERS)
NUM_BATCHES = {"key_ties": 3, "n65537": 2, "chunks3": 3, "key_ties_chunks": 3, "dec_pool": 6, "dec_limits": 5, "dec_lengths": 3}


@functools.lru_cache(maxsize=None)
def case(name: str):
    """(x, y, z, colour, las, kwargs) of a case; the arrays are read-only."""
    x, y, z, c, las, kw = BUILDERS[name]()
    for a in (x, y, z, c):
        assert a.dtype in (np.int32, np.uint32) and a.flags.c_contiguous
        a.setflags(write=False)
    return x, y, z, c, las, kw


@functools.lru_cache(maxsize=None)
def cpu_image(name: str, pad_tails: bool):
    """(image bytes, stats) of the CPU encoder -- the one pinned to the reference -- on a case: what the GPU encoder has to write."""
    x, y, z, c, las, kw = case(name)
    image, st = P.encode_points(x, y, z, c, las, nthreads=2, pad_tails=pad_tails, **kw)
    assert st["num_batches"] == NUM_BATCHES.get(name, 1)
    return bytes(image.view()), st


# ---- the sections of an image -----------------------------------------------------------------------------------------------------
FILE_HEADER = 40                                    # pcr_file_header: five int64
RECORD_HEADER = 20 + 24 + 24 + 48 + 8               # five int32, scale, offset, four float boxes, table size and cluster count
FIXED = (("header", RECORD_HEADER), ("start values", CHAINS * 12), ("separate sizes", CHAINS * 4), ("table values", TABLE * 4),
         ("table lengths", TABLE * 4), ("cluster sizes", CLUSTERS * 4))
SECTIONS = tuple(n for n, _ in FIXED) + ("encoding", "separate", "colours")


def split(image) -> list:
    """The batch records of a .huffman image, each a dict section name -> bytes in the order encode_batch writes them (the record
    header, start values, separate sizes, table values, table lengths, cluster sizes, encoding, separate, colours). The lengths of
    the variable sections are read from the record itself -- the last cluster size, the last separate size -- and cut to the
    record, so a damaged image still splits."""
    data = bytes(image)
    nb = int(np.frombuffer(data[8:16], "<i8")[0]) if len(data) >= FILE_HEADER else 0
    nb = max(0, min(nb, (len(data) - FILE_HEADER) // 8))
    sizes = np.frombuffer(data[FILE_HEADER:FILE_HEADER + 8 * nb], "<i8")
    at, out = FILE_HEADER + 8 * nb, []
    for b in range(nb):
        rec = data[at:at + max(0, int(sizes[b]))]
        at += max(0, int(sizes[b]))
        parts, o = {}, 0
        for name, size in FIXED:
            parts[name] = rec[o:o + size]
            o += size
        last = lambda blob: int(np.frombuffer(blob[-4:], "<i4")[0]) if len(blob) >= 4 else 0
        for name, words in (("encoding", last(parts["cluster sizes"])), ("separate", last(parts["separate sizes"]))):
            size = max(0, min(4 * words, len(rec) - o))
            parts[name] = rec[o:o + size]
            o += size
        parts["colours"] = rec[o:]
        out.append(parts)
    return out


def first_difference(want, got) -> str:
    """'identical', or where `got` leaves `want` first: the file header, the batch sizes, or a batch and the section of its record."""
    want, got = bytes(want), bytes(got)
    if want == got:
        return "identical"
    lengths = f"{len(want)} bytes expected, {len(got)} written; "
    if want[:FILE_HEADER] != got[:FILE_HEADER]:                                 # the totals: said, and the first section still named
        lengths += (f"file header {np.frombuffer(want[:FILE_HEADER], '<i8').tolist()} expected, "
                    f"{np.frombuffer(got[:len(got[:FILE_HEADER]) // 8 * 8], '<i8').tolist()} written; ")
    a, b = split(want), split(got)
    nb = len(a)
    if want[FILE_HEADER:FILE_HEADER + 8 * nb] != got[FILE_HEADER:FILE_HEADER + 8 * nb]:
        lengths += "batch sizes differ; "
    for i, (ra, rb) in enumerate(zip(a, b)):
        for name in SECTIONS:
            sa, sb = ra[name], rb[name]
            if sa == sb:
                continue
            if len(sa) != len(sb):
                return lengths + f"batch {i}, section '{name}': {len(sa)} bytes expected, {len(sb)} written"
            unit = 1 if name in ("header", "colours") else 4
            va, vb = (np.frombuffer(s[:len(s) // unit * unit], f"<u{unit}") for s in (sa, sb))
            d = np.nonzero(va != vb)[0]
            return lengths + (f"batch {i}, section '{name}': {d.size} of {va.size} {'bytes' if unit == 1 else 'words'} differ, first at "
                              f"{int(d[0])} ({int(va[d[0]]):#x} expected, {int(vb[d[0]]):#x} written), last at {int(d[-1])}")
    return lengths + "every section that both images have is equal"


def section(image, b: int, name: str, dtype="<i4") -> np.ndarray:
    return np.frombuffer(split(image)[b][name], dtype)
