"""The inputs of tests/encoder_cases.py are what they claim (tests/test_gpu_encoder_cases.py relies on it): every claim is asserted
here with the CPU encoder -- the one tests/test_ref_pin.py pins to the reference -- and the oracle's loader and decoder. No GPU.

The numpy Morton key is tied to both: a padded-tails stream of `key_ties`, decoded by the oracle, must be the input in
np.lexsort((index, lo, hi)) order. (Only a padded-tails stream decodes to its input; a plain one ends its chains on the
reference's tail artefact.) The Huffman tie rules are restated below as a plain two-queue construction; the whole decoder table the
CPU encoder wrote must be the one it gives, and the shared escape keys are read off it."""
import numpy as np
import pytest

from tests import colour_cases, oracle
from tests import decoder_cases as D
from tests import encoder_cases as E
from tests import select_cases as S

PPB = E.PPB


@pytest.fixture(scope="module")
def files():
    cache = {}

    def get(name, pad):
        if (name, pad) not in cache:
            cache[name, pad] = oracle.OracleFile(E.cpu_image(name, pad)[0])
        return cache[name, pad]
    return get


# ---- the sort ---------------------------------------------------------------------------------------------------------------------
def expected_rows(name: str) -> np.ndarray:
    """int32 [batches x 65536, 3]: the input, chunk by chunk padded with its last point and put in the order of the numpy key."""
    x, y, z, _, _, kw = E.case(name)
    out = []
    for a in range(0, len(x), kw["chunk_points"]):
        part = tuple(v[a:a + kw["chunk_points"]] for v in (x, y, z))
        part = E.padded(part, -(-len(part[0]) // PPB) * PPB)
        order = E.sorted_order(*part)
        out.append(np.stack([v[order] for v in part], axis=1))
    return np.concatenate(out)


@pytest.mark.parametrize("name", ["key_ties", "key_ties_chunks", "n1", "n65536", "n65537", "chunks3"])
def test_sorted_stream_is_the_input_in_the_order_of_the_numpy_key(files, name):
    of = files(name, True)
    want = expected_rows(name)
    assert of.num_batches * PPB == len(want)
    for b in range(of.num_batches):
        rows = S.oracle_points(of, b)
        bad = np.nonzero((rows != want[b * PPB:(b + 1) * PPB]).any(axis=1))[0]
        assert bad.size == 0, f"{name} batch {b}: {bad.size} rows are not where the numpy key puts them, first {bad[0]}"
    print(f"{name}: {of.num_batches} batches decode to the input in np.lexsort((index, lo, hi)) order")


def test_key_ties_counts():
    x, y, z, c, _, _ = E.case("key_ties")
    assert len(x) == E.KEY_TIES_N and len(np.unique(c)) == len(c)
    hi, lo = E.key(x, y, z)
    keys, inv, count = np.unique(np.stack([hi, lo], axis=1), axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    xmin, xmax = np.full(len(keys), 1 << 40), np.full(len(keys), -(1 << 40))
    np.minimum.at(xmin, inv, x.astype(np.int64))
    np.maximum.at(xmax, inv, x.astype(np.int64))
    xs, ys, zs = E.padded((x, y, z), 3 * PPB)
    up, down = E.sorted_order(xs, ys, zs), E.sorted_order(xs, ys, zs, descending_ties=True)
    moved = (np.stack([xs[up], ys[up], zs[up]]) != np.stack([xs[down], ys[down], zs[down]])).any(axis=0)
    got = dict(distinct_keys=len(keys), points_sharing_a_key=int((count[inv] > 1).sum()),
               points_in_groups_that_differ_in_x=int((xmin != xmax)[inv].sum()), distinct_hi=len(np.unique(hi)),
               distinct_lo=len(np.unique(lo)), rows_moved_by_descending_ties=int(moved.sum()))
    print(f"key_ties: {got}")
    assert got == E.KEY_TIES
    # members of a group differ in nothing but X bit 31: the bit the 32-bit `hi` drops
    first = np.zeros(len(keys), np.int64)
    first[inv[::-1]] = np.arange(len(x))[::-1]
    same = lambda v: np.array_equal(v[first[inv]], v)
    assert same(y) and same(z) and same(E.shifted(x) & np.uint64(0x7FFFFFFF))
    # the kinds of neighbours the issue names: sorted keys that differ only in hi, only in bit 63 of lo, only in bits 0 / 1 of hi
    khi, klo = keys[:, 0], keys[:, 1]
    fewer = lambda *cols: len(np.unique(np.stack(cols, axis=1), axis=0)) < len(keys)
    assert fewer(klo, klo) and fewer(khi, klo & ~np.uint64(1 << 63)) and fewer(khi & ~np.uint64(3), klo)


# ---- the Huffman construction, restated -------------------------------------------------------------------------------------------
def two_queue_huffman(freq: dict) -> dict:
    """symbol -> (depth, the first 12 bits of its path) under the encoder's rules: leaves in ascending frequency, ties in ascending
    symbol order; of two equal heads the leaf goes first; the node popped second becomes the left child (bit 0)."""
    syms = sorted(freq)
    leaves = sorted(range(len(syms)), key=lambda i: freq[syms[i]])              # sorted() is stable
    weight = [freq[syms[i]] for i in leaves]
    children = {}
    qa, qb, k = 0, len(leaves), len(leaves)
    def pop():
        nonlocal qa, qb
        if qa < k and (qb >= len(weight) or weight[qa] <= weight[qb]):
            qa += 1
            return qa - 1
        qb += 1
        return qb - 1
    while (k - qa) + (len(weight) - qb) > 1:
        a, b = pop(), pop()
        children[len(weight)] = (b, a)
        weight.append(weight[a] + weight[b])
    out, stack = {}, [(len(weight) - 1, 0, 0)]
    while stack:
        node, prefix, depth = stack.pop()
        if node < k:
            out[syms[leaves[node]]] = (depth, prefix)
            continue
        for bit, child in enumerate(children[node]):
            stack.append((child, prefix << 1 | bit if depth < 12 else prefix, depth + 1))
    return out


def table_from(code: dict):
    """(lengths, values) int32 [4096] as table_from_codes fills them: symbols in ascending order, a later one overwrites."""
    lengths, values = np.zeros(E.TABLE, np.int32), np.zeros(E.TABLE, np.int32)
    for s in sorted(code):
        depth, prefix = code[s]
        rem = 12 - min(depth, 12)
        lengths[prefix << rem:(prefix + 1) << rem] = depth if depth <= 12 else -12
        values[prefix << rem:(prefix + 1) << rem] = s
    return lengths, values


def shared_keys(code: dict) -> dict:
    """12-bit key -> the escaping symbols that share it (two or more)."""
    by_key = {}
    for s, (depth, prefix) in code.items():
        if depth > 12:
            by_key.setdefault(prefix, []).append(s)
    return {k: v for k, v in by_key.items() if len(v) > 1}


def batch_frequencies(name: str) -> dict:
    x, y, z, _, _, _ = E.case(name)
    xyz = np.stack([x, y, z], axis=1).astype(np.int64).reshape(E.CHAINS, E.ROWS, 3)
    d = np.diff(xyz, axis=1, prepend=xyz[:, :1])
    v, n = np.unique(d, return_counts=True)
    return dict(zip(v.tolist(), n.tolist()))


def check_table(of, name):
    """The CPU encoder's table is the restated construction's; returns (code, shared keys)."""
    code = two_queue_huffman(batch_frequencies(name))
    lengths, values = table_from(code)
    cwlen, cwval = E.table_of(of, 0)
    assert np.array_equal(cwlen, lengths), f"{name}: the restated construction gives other code lengths than the CPU encoder"
    assert np.array_equal(cwval, values), f"{name}: the restated construction gives other table values than the CPU encoder"
    shared = shared_keys(code)
    for key, owners in shared.items():
        assert cwlen[key] == -12 and cwval[key] == max(owners), f"{name}: key {key} of {sorted(owners)} belongs to {cwval[key]}"
    return code, shared


@pytest.mark.parametrize("pad", [False, True])
def test_two_symbols(files, pad):
    image, st = E.cpu_image("two_symbols", pad)
    cwlen, values = E.table_of(files("two_symbols", pad), 0)
    print(f"two_symbols {'padded' if pad else 'plain'}: encoded_bytes {st['encoded_bytes']}, escaped {st['escaped_symbols']}, "
          f"values {sorted(set(values.tolist()))}, lengths {sorted(set(cwlen.tolist()))}")
    assert st["encoded_bytes"] == E.TWO_SYMBOLS["encoded_padded" if pad else "encoded_plain"]
    assert st["escaped_symbols"] == E.TWO_SYMBOLS["escaped"]
    assert sorted(set(values.tolist())) == [0, 5] and set(cwlen.tolist()) == {1}
    sizes = E.section(image, 0, "cluster sizes")
    assert np.array_equal(np.diff(sizes, prepend=0), np.full(32, 32 * (8 if pad else 6))), "6 words a chain and no partial word: 8 slots padded"


@pytest.mark.parametrize("name,freqs,symbols,escaped,min_ties", [("fib", E.fib_frequencies(), E.FIB_SYMBOLS, E.FIB_ESCAPED, 1),
                                                                 ("pow2", E.pow2_frequencies(), E.POW2_SYMBOLS, E.POW2_ESCAPED, E.POW2_TERMS - 2)])
def test_leaf_against_internal_ties(files, name, freqs, symbols, escaped, min_ties):
    """`pow2`: the internal node of 1 + 1 + 2 + ... + 2^(k-1) = 2^k meets the leaf 2^k, so every merge but the first is decided by
    `leaves first`. `fib`: the sums 1 + 1 + 2 + 3 + ... are one short of the next leaf, F(k + 2) - 1, so only the first internal
    node (1 + 1 against the leaf 2) ties -- the issue's "every merge" holds for `pow2` alone; which child that first tie makes the
    left one still decides the bits of every deeper code."""
    _, st = E.cpu_image(name, True)
    assert int(freqs.sum()) == symbols and E.batch_frequencies(freqs) == batch_frequencies(name)
    code, shared = check_table(files(name, True), name)
    ties = leaf_internal_ties(batch_frequencies(name))
    deepest = max(d for d, _ in code.values())
    print(f"{name}: escaped_symbols {st['escaped_symbols']}, separate_bytes {st['separate_bytes']}, deepest leaf {deepest}, merges in which "
          f"a leaf ties with an internal node {ties}, shared escape keys {({k: sorted(v) for k, v in shared.items()})}")
    assert st["escaped_symbols"] == escaped and st["separate_bytes"] == 4 * escaped
    assert deepest > 12 and ties >= min_ties and shared, "the tie rules and the owner of a shared key have to decide"
    rare = sorted(batch_frequencies(name).items(), key=lambda kv: kv[1])
    escaping = {s for s, (d, _) in code.items() if d > 12}
    assert sum(batch_frequencies(name)[s] for s in escaping) == escaped and escaping == {s for s, _ in rare[:len(escaping)]}


def leaf_internal_ties(freq: dict) -> int:
    """Pops of the construction at which the leaf queue's head and the internal queue's head have the same weight."""
    w = sorted(freq.values())
    internal, qa, qb, ties = [], 0, 0, 0
    while (len(w) - qa) + (len(internal) - qb) > 1:
        got = []
        for _ in range(2):
            if qa < len(w) and qb < len(internal) and w[qa] == internal[qb]:
                ties += 1
            if qa < len(w) and (qb >= len(internal) or w[qa] <= internal[qb]):
                got.append(w[qa]); qa += 1
            else:
                got.append(internal[qb]); qb += 1
        internal.append(sum(got))
    return ties


def test_flat(files):
    _, st = E.cpu_image("flat", True)
    freq = batch_frequencies("flat")
    assert sum(1 for s, n in freq.items() if n == E.FLAT_TIMES and 1 <= abs(s) <= E.FLAT_VALUES // 2) == E.FLAT_VALUES
    for first, values, times in (E.FLAT_TIED, E.FLAT_IN_TABLE):
        assert all(freq[int(s)] == times for s in E.flat_class(first, values, times))
    assert len(freq) == 1 + E.FLAT_VALUES + E.FLAT_TIED[1] + E.FLAT_IN_TABLE[1]
    code, shared = check_table(files("flat", True), "flat")
    cwlen, _ = E.table_of(files("flat", True), 0)
    in_table = sorted(s for s, (d, _) in code.items() if d <= 12 and s)
    print(f"flat: escaped_symbols {st['escaped_symbols']}, lengths {sorted(set(cwlen.tolist()))}, escape keys {int((cwlen < 0).sum())}, "
          f"of them shared {len(shared)} (by {sum(len(v) for v in shared.values())} symbols), deltas of 12 bits in the table {len(in_table)}, "
          f"merges with a leaf against internal tie {leaf_internal_ties(freq)}")
    assert st["escaped_symbols"] == E.FLAT_ESCAPED and int((cwlen < 0).sum()) == E.FLAT_ESCAPE_KEYS
    assert set(cwlen.tolist()) == {1, 12, -12}, "both sides of the clip"
    assert in_table == sorted(E.flat_class(*E.FLAT_IN_TABLE).tolist())
    assert len(shared) == E.FLAT_ESCAPE_KEYS and leaf_internal_ties(freq) >= E.FLAT_TIED[1]


@pytest.mark.parametrize("pad", [False, True])
def test_mixed_lanes(files, pad):
    image, st = E.cpu_image("mixed_lanes", pad)
    of = files("mixed_lanes", pad)
    cwlen, values = E.table_of(of, 0)
    length = {int(v): int(l) for v, l in zip(values[cwlen > 0].tolist(), cwlen[cwlen > 0].tolist())}
    d = E.mixed_lanes_deltas().reshape(E.CHAINS, 192)
    bits = np.array([[length.get(int(s), 12) for s in row] for row in d]).sum(axis=1).reshape(E.CLUSTERS, E.LANES)
    escapes = np.diff(D.separate_sizes(of, 0), prepend=0).reshape(E.CLUSTERS, E.LANES)
    words = -(-bits // 32)
    print(f"mixed_lanes {'padded' if pad else 'plain'}: escaped {st['escaped_symbols']}, bits a chain {int(bits.min())} / {int(bits.max())}, words "
          f"{int(words.min())} / {int(words.max())}, escapes a chain {int(escapes.min())} / {int(escapes.max())}, encoded_bytes {st['encoded_bytes']}")
    assert st["escaped_symbols"] == E.MIXED_ESCAPED
    assert (bits[:, 0::2] == E.MIXED_BITS[0]).all() and (bits[:, 1::2] == E.MIXED_BITS[1]).all(), "the extremes alternate lane by lane in every cluster"
    assert (escapes[:, 0::2] == 0).all() and (escapes[:, 1::2] == 189).all()
    slots = words + (np.where(bits % 32 == 0, 2, 1) if pad else 0)               # padded: a zero word for every refill that finds none
    assert np.array_equal(np.diff(E.section(image, 0, "cluster sizes"), prepend=0), slots.sum(axis=1))


def test_colours():
    blocks = E.colour_blocks()
    assert blocks.shape == (E.COLOUR_BLOCKS, 16) and (blocks[:E.TWIN_FIRST] >> 24 == 0).all()
    k = np.arange(E.TWINS)
    twins, early = blocks[E.TWIN_FIRST + k], blocks[E.twin_of(k)]
    assert (twins >> 24 == 0xFF).all() and np.array_equal(twins & 0xFFFFFF, early)
    for pad in (False, True):
        bc1 = E.section(E.cpu_image("colours", pad)[0], 0, "colours", np.uint8).reshape(E.COLOUR_BLOCKS, 8)
        a, b = bc1[E.TWIN_FIRST + k], bc1[E.twin_of(k)]
        assert np.array_equal(colour_cases.spec_bc1(a), colour_cases.spec_bc1(b)) and np.array_equal(a, b), "the encoder reads 24 bits"
        ref = np.load(colour_cases.G + "/bc1_ref_blocks.npz")["blocks"]
        same = int((bc1[:256] == ref).all(axis=1).sum())
        uniform = bc1[256:768, 4:]
        print(f"colours: {len(np.unique(bc1, axis=0))} distinct blocks of {len(bc1)}; {same} of the reference's 256 blocks reproduced; "
              f"selector bytes of the 512 one-colour blocks {sorted(set(uniform.reshape(-1).tolist()))}")
        assert (uniform == uniform[:, :1]).all(), "a one-colour block has one selector"


# ---- the streams of decoder_cases -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("name", D.STREAMS)
def test_decoder_streams_are_their_own_images(name, pad):
    image, st = E.cpu_image(f"dec_{name}", pad)
    assert E.first_difference(bytes(E.decoder_stream(name, pad)), image) == "identical"
    print(f"dec_{name} {'padded' if pad else 'plain'}: {st['num_batches']} batches, {len(image)} bytes")


# ---- the splitter -----------------------------------------------------------------------------------------------------------------
def test_sections_tile_the_record_and_name_a_difference():
    image, _ = E.cpu_image("dec_lengths", True)
    recs = E.split(image)
    assert len(recs) == 3 and list(recs[0]) == list(E.SECTIONS)
    body = b"".join(r[n] for r in recs for n in E.SECTIONS)
    assert image[E.FILE_HEADER + 8 * 3:] == body
    assert all(len(r["colours"]) == PPB // 2 for r in recs) and len(recs[1]["encoding"]) and len(recs[1]["separate"])
    assert E.first_difference(image, image) == "identical"
    at = E.FILE_HEADER + 8 * 3 + sum(len(recs[0][n]) for n in E.SECTIONS)      # batch 1
    for name in E.SECTIONS:
        damaged = bytearray(image)
        damaged[at + len(recs[1][name]) // 2] ^= 0x40
        said = E.first_difference(image, bytes(damaged))
        assert f"batch 1, section '{name}'" in said, said
        at += len(recs[1][name])
    assert "file header" in E.first_difference(image, image[:8] + b"\7" + image[9:])
    assert "batch 2, section 'colours'" in E.first_difference(image, image[:-5])
    said = E.first_difference(E.cpu_image("two_symbols", True)[0], E.cpu_image("two_symbols", False)[0])       # other totals, other sizes
    assert "file header" in said and "batch 0, section 'cluster sizes'" in said, said
