"""The streams of tests/decoder_cases.py are what they claim (tests/test_gpu_decoder.py relies on it): every claim is asserted here
from walk(), the numpy restatement of one batch's decode, which is itself held against the oracle's decoder and its lane words for
every stream -- so the census below is a census of the decode the oracle pins to the reference. No GPU.

The claims are about the streams as designed: they are asserted for the padded streams (and their BC7 twins, the same rows). The plain
streams are the same rows under the reference's tail artefact, which rewrites the last symbols of low-entropy chains; for them the
walk is tied to the oracle in the same way and the census is printed. What cannot be built is asserted as impossible instead:
  * row 0 of a chain is three codes of delta 0. 3072 of a batch's 196 608 symbols are that delta, a code's length under a Huffman
    code is below log(1 / p) / log(golden ratio) + 1 = 9.7 for p = 1 / 64, so row 0 has at most 27 bits: points of more than 32
    bits are demanded in rows 1, 62 and 63 and row 0 is asserted to stay below;
  * a point of b = 3 .. 36 bits that starts at offset o retires (o + b) // 32 words: none only for o <= 28, two only for o >= 28,
    one at every offset. FEASIBLE below is that set, all of it is demanded, and nothing outside it occurs;
  * a batch of more than 2 * 5120 escape words has a half over its pool: the first two batches of `pool` are (0, 1), not (0, 0)."""
import numpy as np
import pytest

from tests import decoder_cases as D

PADDED = [v for v in D.VARIANTS if v[1]]
FEASIBLE = {(o, r) for o in range(32) for b in range(3, 37) for r in [(o + b) // 32]}


def ids(vs):
    return [D.variant_id(v) for v in vs]


def of_variant(v, names):
    return [x for x in v if x[0] in names]


# ---- the restated rule is the kernels' --------------------------------------------------------------------------------------------
def test_constants_and_rule_are_the_kernels():
    """A changed pool size, slack, sentinel or comparison fails here instead of silently moving the boundaries the streams sit on."""
    text = D.kernel_source()
    assert D.source_constants(text) == dict(ESC_POOL_WORDS=D.ESC_POOL_WORDS, ESC_POOL_WORDS_HALF=D.ESC_POOL_WORDS_HALF, ESC_SLACK=D.ESC_SLACK,
                                            TE_SLOW_VALUE=D.TE_SLOW_VALUE, TE_VALUE_SHIFT=D.TE_VALUE_SHIFT)
    for line in D.RULE_TEXT:
        assert text.count(line) == 1, f"the kernel source no longer says `{line}`"
    assert D.LIMIT == -D.TE_SLOW_VALUE and 32 - D.TE_VALUE_SHIFT == 22, "a signed 22-bit value whose most negative number is the sentinel"
    assert FEASIBLE == {(o, 0) for o in range(29)} | {(o, 1) for o in range(32)} | {(o, 2) for o in range(28, 32)}


# ---- the walk is the oracle's decode ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", D.VARIANTS, ids=ids(D.VARIANTS))
def test_walk_is_the_oracles_decode(v):
    of, ws, rows = D.oracle_file(*v), D.walks(*v), D.points(v[0])
    assert of.num_batches == len(rows) == len(ws)
    for b, w in enumerate(ws):
        dec = of.decode_batch(b)
        assert np.array_equal(w["xyz"], dec), f"batch {b}: the walk decodes other points than the oracle"
        assert np.array_equal(w["words"], w["lane_counts"]), f"batch {b}: the walk's word counts are not lane_words' counts"
        garbage = int((dec.reshape(-1, 3) != rows[b]).any(axis=1).sum())
        cwlen, _ = D.table_of(of, b)
        print(f"{D.variant_id(v)} batch {b}: lengths {sorted(set(cwlen.tolist()))}, escape words read {int(w['esc_words'].sum())} "
              f"(written {int(w['separate_sizes'][1023])}), words a chain {int(w['words'].min())} .. {int(w['words'].max())}, bits a point "
              f"{int(w['bits'].min())} .. {int(w['bits'].max())}, flags {D.expected_flags(of, b, w)}, rows that differ from the input {garbage}")
        assert w["bits"].min() >= 3 and w["bits"].max() <= 36
        if v[1]:
            assert garbage == 0, "a padded stream decodes to the rows given"
            assert np.array_equal(w["esc_words"], np.diff(w["separate_sizes"], prepend=0)), "a padded chain reads the escapes written for it"


# ---- phases -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", of_variant(PADDED, ("phases",)), ids=ids(of_variant(PADDED, ("phases",))))
def test_phases(v):
    """Measured (padded): 12 in-table lengths and one escape key of 12 bits; every (offset, words retired) pair of FEASIBLE, 65 of
    them; 3-bit and 36-bit points at all 32 offsets; 400 escapes."""
    of, (w,) = D.oracle_file(*v), D.walks(*v)
    cwlen, values = D.table_of(of, 0)
    assert set(cwlen.tolist()) == set(range(1, 13)) | {-12}
    for k, val in D.PHASES_VALUE.items():
        assert set(cwlen[values == val].tolist()) >= {k}, f"delta {val} was to have a code of {k} bits"
    # every length and the escape as first, second and third symbol
    cls = np.where(w["escape"], D.ESC, w["length"]).reshape(D.CHAINS, D.ROWS, 3)
    census = np.array([[int((cls[:, :, k] == c).sum()) for k in range(3)] for c in range(1, 14)])
    print("phases: points with class c (1 .. 12, escape) as symbol 0 / 1 / 2:\n" + str(census))
    assert (census > 0).all(), f"a class never occurs in a position:\n{census}"
    assert np.array_equal(cls, D.phases_plan()), "the table gives other lengths than the plan asked for"
    # offsets against words retired
    pairs = {}
    for o, r in zip(w["offset"].reshape(-1).tolist(), w["retired"].reshape(-1).tolist()):
        pairs[(o, r)] = pairs.get((o, r), 0) + 1
    print("phases: points per (offset, words retired): " + ", ".join(f"{k}: {n}" for k, n in sorted(pairs.items())))
    assert set(pairs) == FEASIBLE, f"missing {sorted(FEASIBLE - set(pairs))}, impossible {sorted(set(pairs) - FEASIBLE)}"
    for bits in (3, 36):
        at = np.bincount(w["offset"][w["bits"] == bits], minlength=32)
        print(f"phases: {bits}-bit points per offset: {at.tolist()}")
        assert (at > 0).all(), f"no {bits}-bit point at offsets {np.nonzero(at == 0)[0].tolist()}"
    # the low plane of the 40-bit windows: points that reach past bit 32 of their own window
    over = (w["bits"] > 32).sum(axis=0)
    print(f"phases: points of more than 32 bits per row: {over.tolist()}")
    assert over[1] > 0 and over[62] > 0 and over[63] > 0
    assert (w["bits"][:, 0] == 3 * int(cwlen[values == 0].max())).all() and w["bits"][:, 0].max() <= 27
    assert (w["n_escapes"][w["bits"] == 36] == 3).any() and (w["n_escapes"][w["bits"] == 36] == 0).any(), "36 bits from escapes and from codes of 12"
    assert D.expected_flags(of, 0, w) == (0, 0)


# ---- runs ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", of_variant(PADDED, ("runs",)), ids=ids(of_variant(PADDED, ("runs",))))
def test_runs(v):
    """Measured (padded): all 16 (previous, this) pairs; all 8 patterns wave-uniform and lane-divergent; chain 200 escapes whole;
    6333 escape words, 3261 + 3072 by halves: unflagged."""
    of, (w,) = D.oracle_file(*v), D.walks(*v)
    n = w["n_escapes"]
    pairs = np.zeros((4, 4), np.int64)
    np.add.at(pairs, (n[:, :-1].reshape(-1), n[:, 1:].reshape(-1)), 1)
    print("runs: points per (escapes of the previous point, escapes of this point):\n" + str(pairs))
    assert (pairs > 0).all()
    e = w["escape"].reshape(D.CHAINS, D.ROWS, 3)
    pattern = (e[:, :, 0] + 2 * e[:, :, 1] + 4 * e[:, :, 2]).reshape(D.CHAINS // 64, 64, D.ROWS)      # [wave, lane, row]
    uniform = (pattern == pattern[:, :1]).all(axis=1)                                                # [wave, row]
    divergent = (pattern[:, 1:] != pattern[:, :-1]).all(axis=1)                                      # every lane differs from its neighbour
    for p in range(8):
        u = int((uniform & (pattern[:, 0] == p)).sum())
        d = int((divergent[:, None, :] & (pattern == p)).any(axis=1).sum())
        print(f"runs: pattern {p:03b}: wave-uniform at {u} (wave, row) places, among lanes that all differ from their neighbours at {d}")
        assert u > 0 and d > 0
    whole = np.nonzero(w["escape"][:, 3:].all(axis=1))[0]
    assert whole.tolist() == [D.RUNS_ALL_ESCAPING] and w["esc_words"][D.RUNS_ALL_ESCAPING] == 189 and w["words"][D.RUNS_ALL_ESCAPING] == D.LONG_WORDS
    # lanes of one wave differ in (esc_prev, n): wave 2
    assert len({(int(a), int(b)) for a, b in zip(n[128:192, 3], n[128:192, 4])}) == 1 and len({tuple(r) for r in e[128:192, 4].tolist()}) == 3
    assert D.expected_flags(of, 0, w) == (0, 0) and int(w["esc_words"][:512].sum()) <= D.ESC_POOL_WORDS_HALF >= int(w["esc_words"][512:].sum())
    cwlen, _ = D.table_of(of, 0)
    assert set(cwlen.tolist()) == {1, -12}


# ---- pool ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", of_variant(D.VARIANTS, ("pool",)), ids=ids(of_variant(D.VARIANTS, ("pool",))))
def test_pool(v):
    """Measured (padded and plain alike: the chains' tails are zero bits and so is what the artefact hands them): escape words read
    13248, 13312, 13313 by the whole batch; 5120, 5121 by chains 0 .. 511 and 5121 by chains 512 .. 1023 of batches of 5420 and 5421;
    the first word behind a pool is the third escape of a point of three."""
    of, ws = D.oracle_file(*v), D.walks(*v)
    for b, w in enumerate(ws):
        halves = (int(w["esc_words"][:512].sum()), int(w["esc_words"][512:].sum()))
        reach = int((w["first_esc"] + w["esc_words"]).max())
        flags = D.expected_flags(of, b, w)
        cross = [D.crossing(w, part) for part in (None, 0, 1)]
        print(f"pool batch {b}: escape words by halves {halves}, the farthest word read {reach}, flags {flags}, crossings (whole, half 0, half 1) {cross}")
        assert halves == D.POOL_HALVES[b] and reach == sum(halves) == D.POOL_TOTALS[b]
        assert flags == D.POOL_FLAGS[b] and not D.has_wide_value(of, b)
        for part, over in zip((None, 0, 1), (D.POOL_TOTALS[b] > D.ESC_POOL_WORDS, halves[0] > D.ESC_POOL_WORDS_HALF, halves[1] > D.ESC_POOL_WORDS_HALF)):
            assert (D.crossing(w, part) is not None) == over
    assert D.POOL_TOTALS[:3] == (D.ESC_POOL_WORDS - D.ESC_SLACK, D.ESC_POOL_WORDS, D.ESC_POOL_WORDS + 1)
    assert [h[0] for h in D.POOL_HALVES[3:5]] == [D.ESC_POOL_WORDS_HALF, D.ESC_POOL_WORDS_HALF + 1] and D.POOL_HALVES[5][1] == D.ESC_POOL_WORDS_HALF + 1
    # the batches the claim is about cross inside a point of three
    for b, part in ((2, None), (4, 0), (5, 1)):
        c = D.crossing(ws[b], part)
        assert c is not None and c[2] == 3 and c[3] > 0


# ---- limits -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", of_variant(D.VARIANTS, ("limits",)), ids=ids(of_variant(D.VARIANTS, ("limits",))))
def test_limits(v):
    """Measured: batch 0 has seven table values, lengths 2 and 3, no escape key; batch 1 the same seven, one-off deltas with codes of
    12 bits and 88 escape words; batch 2 the values 0 and +-(2^21 - 1), lengths 1 and 2; batches 3 and 4 those and 2^21, or
    -2^21, 48 times a chain at most."""
    of, ws = D.oracle_file(*v), D.walks(*v)
    seven = set(D.LIMIT_VALUES) | {0}
    for b, w in enumerate(ws):
        cwlen, values = D.table_of(of, b)
        in_table = set(values[cwlen > 0].tolist())
        escapes = int(w["esc_words"].sum())
        flags = D.expected_flags(of, b, w)
        print(f"limits batch {b}: {len(in_table)} table values, escape keys {int((cwlen <= 0).sum())}, escape words {escapes}, flags {flags}")
        assert flags == D.LIMITS_FLAGS[b]
        over = D.crossing(w, None), D.crossing(w, 0), D.crossing(w, 1)
        assert over == (None, None, None), "no batch here is over a pool: only the wide entries can flag it"
        if b == 0:
            assert in_table == seven and (cwlen > 0).all() and escapes == 0
        elif b == 1:
            assert in_table >= seven and escapes > 0 and (cwlen <= 0).any()
        elif b == 2:
            assert in_table == {0, D.LIMIT - 1, -(D.LIMIT - 1)} and (cwlen > 0).all()
        else:
            only = D.LIMIT if b == 3 else -D.LIMIT
            assert in_table == {0, D.LIMIT - 1, -(D.LIMIT - 1), only} and (cwlen > 0).all()
            most = int((w["delta"] == only).sum(axis=1).max())
            print(f"limits batch {b}: the one wide value {only} occurs at most {most} times a chain")
            assert 0 < most <= D.ESC_SLACK
        used = set(w["delta"][~w["escape"]].tolist())
        assert used >= (seven if b < 2 else in_table), "every value is decoded from the table somewhere"
    assert [bool(D.value_fits(x)) for x in D.LIMIT_VALUES] == [True, True, False, False, False, False]


# ---- lengths ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", of_variant(D.VARIANTS, ("lengths",)), ids=ids(of_variant(D.VARIANTS, ("lengths",))))
def test_lengths(v):
    """Measured: batch 0 every key of the table has length 1 and every chain 8 words; batches 1 and 2 eight waves of 8-word chains and
    eight of 72-word chains, 96 768 escape words."""
    of, ws = D.oracle_file(*v), D.walks(*v)
    cwlen, values = D.table_of(of, 0)
    assert (cwlen == 1).all() and (values == 0).all() and (ws[0]["words"] == D.SHORT_WORDS).all() and D.SHORT_WORDS == 8
    assert (of.decode_batch(0).reshape(-1, 3) == [7, -3, 11]).all()
    for b in (1, 2):
        per_wave = ws[b]["words"].reshape(D.CHAINS // 64, 64)
        long = D.long_waves(b)
        print(f"lengths batch {b}: words a chain by wave {[(int(r.min()), int(r.max())) for r in per_wave]}")
        for wave in range(D.CHAINS // 64):
            if wave in long:
                assert (per_wave[wave] >= D.LONG_WORDS).all() and D.LONG_WORDS == 72
            else:
                assert (per_wave[wave] == D.SHORT_WORDS).all()
        assert ((D.CHAINS // 64 - 1) in long) == (b == 1), "batch 1 ends on a long wave, batch 2 on a short one"
        assert len(long) == 8 and all((w + 1) % 16 not in long for w in long)


# ---- the cameras --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", D.STREAMS)
def test_cameras_see_the_stream(name):
    """The near frame walks every point and at least half of every batch's are inside; the far one draws every batch with npr < 64."""
    near, far = D.cameras(name)
    assert (near.width, near.height) == (D.WIDTH, D.HEIGHT) == (320, 200)
    for pad in (True, False):
        of = D.oracle_file(name, pad)
        for b in range(of.num_batches):
            drawn, npr, _ = of.batch_lod(b, near)
            inside = len(of.trace_points(near, first=b, count=1)[0])
            fdrawn, fnpr, _ = of.batch_lod(b, far)
            print(f"{name} {'padded' if pad else 'plain'} batch {b}: near npr {npr}, {inside} inside; far npr {fnpr}")
            assert drawn and npr == 64 and 2 * inside >= D.PPB
            assert fdrawn and 0 < fnpr < 64
