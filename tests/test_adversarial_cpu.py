"""The adversarial streams of tests/adversarial_cases.py, the parts that need no GPU: the restated lattice, key and home slot pinned
to the sources, and, from the oracle's decode of every stream, the proof that it is as hard as tests/test_gpu_adversarial.py takes
it to be. Every test prints the counts behind its assertions.

The counts the oracle's decode gave when the streams were built:
  collide, cell / radius 4, no clip: 65 536 runs, 131 072 slots, 585 voxels.
    thin lattice   256 keys on home 131 069, the run of occupied slots through it starts at 131 069 and is 257 long: it wraps, and
                   253 keys sit behind slot 0 (found only by a probe that wraps).
    noise lattice  256 keys on home 131 069, run 131 069 + 272: it wraps, 257 keys behind slot 0; 16 foreign keys inside it, all 16
                   displaced when inserted in row order; 28 lookups of absent keys inside it, 15 of them across the wrap, the longest
                   past 272 occupied slots; 285 occupied neighbour pairs with one end on the shared home. (A second run of 256 keys,
                   T seen through the noise lattice, lies away from the table's end.)
  collide, clip x <= 1023: 31 278 runs, 65 536 slots, 276 voxels; thin: 126 keys on home 65 534, run 65 534 + 127, wraps, 124 keys
    behind slot 0; noise: 125 keys on home 65 534, run 65 534 + 129, wraps, 125 behind slot 0; 4 foreign keys, 8 absent lookups
    inside it, 4 across the wrap.
  edges64, radius 64: 55 703 voxels, 55 839 work items, pairs_bound 33 805 962; lone voxels of 1, 63, 64, 65, 127, 128, 129, 4096 and
    4097 rows; 13 voxels with an interior bucket end on a tile end, 2 with a bucket over three tiles; totals of 64 or more by total
    mod 64: 13, 8, 2, 2; min_count 64 / 65 / 128 / 129 splits 6 / 7 / 3 / 2 single work items and leaves 16 / 11 / 4 / 3 voxels wholly
    kept; 358 rows whose N lies strictly between their voxel's count and their N27.
  moments_limit, r = 32767: the 64 rows at the origin have q_xx = q_yy = q_zz >= 64 * 32767^2, the far clusters s <= -64 * 32767.
  neighbors_limit, r = 2^20: 6 ordered pairs at exactly r, 2 more with nn2 = 2^40 - 447, 3 rows without a neighbour.
  shapes, cell 8: 3 components under 26, 4097 under 6; the path has 8255 voxels and 61 440 rows, its ends are 8254 (6) and 8128 (26)
    steps apart."""
import functools
import os

import numpy as np
import pytest

from pcrhpg24_amd import build
from tests import adversarial_cases as A
from tests import components_cases as K
from tests import denoise_cases as D
from tests import moments_cases as MC
from tests import neighbors_cases as NC
from tests import oracle
from tests import select_cases as S
from tests import thin_cases as T
from tests.test_thin_cpu import LATTICE_CASES, lattice_by_hand


# ---- the restatement is the source's -----------------------------------------------------------------------------------------------
def test_hash_is_the_kernels():
    """A changed multiplier or a fifth (or a missing) copy of the probe loop fails here instead of silently emptying the cases."""
    text = open(os.path.join(build.CSRC, "pcr_kernels.hip.h")).read()
    assert f"THIN_HASH_MUL = 0x{A.HASH_MUL:016X}ull;" in text
    assert text.count(A.HASH_TEXT) == 4, "one home-slot expression per probe function: thin_insert, denoise_insert_slot, denoise_lookup, components_lookup"
    assert "THIN_KEY_BITS = %d;" % A.KEY_BITS in open(os.path.join(build.CSRC, "pcr_lattice.h")).read()
    assert A.KEY_BITS == T.KEY_BITS and A.HASH_MUL % 2 == 1
    keys = np.array([0, 1, 1 << 21, 1 << 42, (1 << 63) - 1, A.key_of((513, 2, 77))], np.uint64)
    for log2 in (10, 16, 17, 22):
        assert [int(h) for h in A.homes_of(keys, log2)] == [A.home_of(int(k), log2) for k in keys]
    assert [int(k) for k in A.keys_of(np.array([[513, 2, 77], [0, 0, 1]]))] == [A.key_of((513, 2, 77)), 1 << 42]


def test_lattice_shift_is_thin_lattice_and_one_cell_more():
    done = 0
    for origin, cell, lo, hi in LATTICE_CASES:
        want = lattice_by_hand(origin, cell, lo, hi)
        if want[0] != 0:
            continue
        thin, noise = A.lattice_origin(origin, cell, lo), A.lattice_origin(origin, cell, lo, 1)
        assert [v % (1 << 32) for v in thin] == want[2:5]
        assert all(t - n == cell for t, n in zip(thin, noise))
        assert A.voxel_of(lo, thin, cell) == (0, 0, 0) and A.voxel_of(lo, noise, cell) == (1, 1, 1)
        done += 1
    assert done >= 8


def test_every_property_is_demanded_by_a_case():
    assert set(A.CASES) == set(A.STREAMS)
    assert set(A.PROPERTIES) == {k for needs in A.CASES.values() for k in needs}
    assert sum(len(v) for v in A.CASES.values()) == len(A.PROPERTIES), "a property belongs to one stream"


def demand(name, got):
    print(f"{name}: " + ", ".join(f"{k} {got[k]}" for k in A.CASES[name]))
    for k in A.CASES[name]:
        assert got[k] >= 1, f"{name}: {k} does not occur"


# ---- the decode is the rows given ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_rows(name):
    of = oracle.OracleFile(A.stream(name))
    assert of.num_batches == 1
    return S.oracle_points(of, 0).astype(np.int64), S.oracle_bounds(of)


@pytest.mark.parametrize("name", A.STREAMS)
def test_decode_equals_the_rows_given(name):
    xyz, bounds = oracle_rows(name)
    assert xyz.shape == (A.PPB, 3) and np.array_equal(xyz, A.points(name)), "the oracle does not decode the rows the case was built from"
    assert np.array_equal(bounds[0], np.concatenate([xyz.min(axis=0), xyz.max(axis=0)]))


# ---- collide -----------------------------------------------------------------------------------------------------------------------
def collide_reports(clip):
    xyz, bounds = oracle_rows("collide")
    cell = A.COLLIDE_CELL
    vox = (0, 0, 0, cell)
    assert T.lattice_refusal(bounds, vox, clip) is None and D.lattice_refusal(bounds, vox, clip) is None and NC.lattice_refusal(bounds, cell, clip) is None
    runs = T.count_runs(xyz, vox, clip)
    assert runs == NC.count_runs(xyz, cell, clip) == int(T.candidates(xyz, clip).sum()), "a row is not a run of its own"
    slots = T.table_slots(runs)
    log2 = A.log2_of(slots)
    home = A.COLLIDE_HOME >> (A.log2_of(A.COLLIDE_SLOTS) - log2)        # (the home is the product's top bits: one bit less, half the slot)
    reports = []
    for more in (0, 1):
        keys, voxels = A.occupied_keys(xyz, cell, more, clip)
        assert tuple(voxels[0]) == (more,) * 3, "the pin does not hold the lattice"
        reports.append(A.cluster_report(keys, voxels, log2, more == 1, home))
    return runs, slots, reports


def test_collide_plan():
    plan = A.collide_plan()
    print("collide plan: " + ", ".join(f"{k} {len(v) if isinstance(v, list) else v}" for k, v in plan.items()))
    log2 = A.log2_of(A.COLLIDE_SLOTS)
    assert all(A.home_of(A.key_of(v), log2) == A.COLLIDE_HOME for v in plan["T"])
    assert all(A.home_of(A.key_of(tuple(c + 1 for c in v)), log2) == A.COLLIDE_HOME for v in plan["N"])
    for v in plan["displaced"] + plan["absent"]:
        assert (A.home_of(A.key_of(tuple(c + 1 for c in v)), log2) - A.COLLIDE_HOME) % A.COLLIDE_SLOTS <= A.COLLIDE_WINDOW
    occupied = set(plan["order"])
    assert not occupied & set(plan["absent"]) and all((v[0] + 1, v[1], v[2]) in occupied for v in plan["absent"])
    assert min(min(v) for v in plan["order"]) == 0 and plan["order"][0] == (0, 0, 0)
    xyz = A.points("collide")
    assert {tuple(v) for v in (xyz // A.COLLIDE_CELL).tolist()} == occupied
    copies = np.unique(xyz, axis=0, return_counts=True)[1]
    assert (copies > 1).any() and (copies == 1).any(), "exact duplicates and single rows"


def test_collide_is_one_cluster_that_wraps_the_table():
    runs, slots, (thin, noise) = collide_reports(None)
    print(f"collide: {runs} runs, {slots} slots\n  thin lattice:  {thin}\n  noise lattice: {noise}")
    assert runs == A.PPB and slots == A.COLLIDE_SLOTS
    for rep in (thin, noise):
        assert rep["home"] == A.COLLIDE_HOME and rep["shared"] >= 256
        assert rep["wraps"] and rep["first"] <= rep["home"] and rep["first"] + rep["length"] >= slots + rep["shared"] - 3
        assert rep["found_across_wrap"] >= rep["shared"] - 3           # all but the three slots before the table's end
    assert noise["foreign"] >= 8 and noise["displaced"] >= 8
    assert noise["absent_in_cluster"] >= 8 and noise["absent_across_wrap"] >= 1 and noise["longest_absent_walk"] >= 256
    assert noise["pairs_with_cluster"] >= 32
    demand("collide", dict(shared_home=min(thin["shared"], noise["shared"]) >= 256, wraps=thin["wraps"] and noise["wraps"], found_across_wrap=min(thin["found_across_wrap"], noise["found_across_wrap"]),
                           displaced=noise["displaced"],
                           absent_in_cluster=noise["absent_in_cluster"], absent_across_wrap=noise["absent_across_wrap"],
                           pairs_with_cluster=noise["pairs_with_cluster"], clipped_wraps=all(r["wraps"] for r in collide_reports(A.COLLIDE_CLIP)[2])))


def test_collide_with_the_clip_is_shorter_and_still_wraps():
    xyz, _ = oracle_rows("collide")
    plan = A.collide_plan()
    kept = lambda vs: sum(v[0] * A.COLLIDE_CELL + A.COLLIDE_CELL - 1 <= A.COLLIDE_CLIP[1][0] for v in vs)
    runs, slots, (thin, noise) = collide_reports(A.COLLIDE_CLIP)
    print(f"collide, clip {A.COLLIDE_CLIP}: {runs} runs, {slots} slots, {kept(plan['T'])} of T and {kept(plan['N'])} of N left\n  thin lattice:  {thin}\n  noise lattice: {noise}")
    assert 64 <= kept(plan["T"]) <= 192 and 64 <= kept(plan["N"]) <= 192
    assert 0 < runs < A.PPB and slots == A.COLLIDE_CLIP_SLOTS
    assert thin["shared"] == kept(plan["T"]) and noise["shared"] == kept(plan["N"])
    for rep in (thin, noise):
        assert rep["wraps"] and 64 <= rep["length"] < 256 and rep["found_across_wrap"] >= 64
    assert noise["absent_across_wrap"] >= 1
    # every voxel lies on one side of the clip: a voxel's rows are all candidates or none is
    inside = S.in_box(xyz, A.COLLIDE_CLIP)
    v = xyz // A.COLLIDE_CELL
    key = A.keys_of(v)
    assert len(np.intersect1d(key[inside], key[~inside])) == 0


# ---- edges64 -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edges64():
    xyz, bounds = oracle_rows("edges64")
    assert NC.lattice_refusal(bounds, A.EDGE_CELL) is None
    an = NC.analyse(xyz, A.EDGE_CELL)
    assert np.array_equal(an["rows"], np.arange(A.PPB)) and an["pairs"] < 3e7
    return xyz, an, A.bucket_layout(xyz, A.EDGE_CELL)


def test_edges64_populations_tiles_and_thresholds():
    xyz, an, (vox, lengths, which) = edges64()
    own, total = lengths[:, 13], lengths.sum(axis=1)
    ends = np.cumsum(lengths, axis=1)
    starts = ends - lengths
    filled = lengths > 0
    assert np.array_equal(total[which], an["n27"]) and int((own * total).sum()) == an["pairs_bound"]
    print(f"edges64: {len(vox)} voxels, {int(((own + 63) // 64).sum())} work items, pairs_bound {an['pairs_bound']}, {an['pairs']} pairs of distinct points, "
          f"runs {NC.count_runs(xyz, A.EDGE_CELL)}")
    got = {}
    lone = {c: int(((own == c) & (total == c)).sum()) for c in A.LONE}
    print(f"  lone voxels by population: {lone}")
    got["populations"] = min(lone.values())
    on_tile = filled & (ends % 64 == 0) & (ends < total[:, None])
    got["bucket_on_tile"] = int(on_tile.any(axis=1).sum())
    three = filled & (starts % 64 != 0) & ((ends - 1) // 64 - starts // 64 >= 2)
    got["bucket_three_tiles"] = int(three.any(axis=1).sum())
    for what in ("face 63|1|64", "edge 64|64", "corner 1|126|1", "three tiles 32|130|30"):
        sizes = sorted(int(own[(vox - vox.min(axis=0) == np.array(v) - xyz.min(axis=0) // A.EDGE_CELL).all(axis=1)][0]) for w, v, _ in A.edges64_plan() if w == what)
        assert sizes == sorted(int(s) for s in what.split()[-1].split("|")), what
    mod = {m: int(((total >= 64) & (total % 64 == m)).sum()) for m in range(4)}
    print(f"  voxels with an interior bucket end on a tile end: {got['bucket_on_tile']}, with a bucket over three tiles: {got['bucket_three_tiles']}, "
          f"neighbourhood totals of 64 or more by total mod 64: {mod}")
    got["totals_mod_64"] = min(mod.values())
    # N per voxel: the least and the greatest over its centres
    n = an["n"]
    least, most = np.full(len(vox), np.iinfo(np.int64).max), np.zeros(len(vox), np.int64)
    np.minimum.at(least, which, n)
    np.maximum.at(most, which, n)
    split = {k: (int(((own <= 64) & (least < k) & (most >= k)).sum()), int((least >= k).sum()), int((most < k).sum())) for k in A.THRESHOLDS}
    print(f"  min_count: (single work items it splits, voxels wholly kept, voxels wholly sparse) {split}")
    got["thresholds_split"] = min(min(v) for v in split.values())
    # a compact lone voxel of 128 or 129 rows: whatever the order of its bucket, after the first tile every centre has exactly 64
    compact = (total == own) & (least == own) & np.isin(own, (128, 129))
    got["exit_on_tile"] = int(compact.sum())
    got["sphere_decides"] = int(((n > own[which]) & (n < an["n27"])).sum())
    assert ((an["nn2"] == 0).sum() > 1000) and ((an["nn2"] == NC.NONE).sum() > 1000) and ((an["nn2"] != 0) & (an["nn2"] != NC.NONE)).sum() > 1000
    demand("edges64", got)


def test_edges64_through_the_other_calls():
    """pcr_denoise and pcr_components at cell 64: both classes occur at the medians tests/test_gpu_adversarial.py uses."""
    xyz, _ = oracle_rows("edges64")
    vox = (0, 0, 0, A.EDGE_CELL)
    an = D.analyse(xyz, vox)
    median = D.median_n27(an)
    assert 0 < (an["n27"] <= median).sum() < A.PPB
    for conn in (6, 26):
        comp = K.analyse(xyz, vox, None, conn)
        k = max(K.median_size(comp), 2)
        print(f"edges64 cell 64 conn {conn}: median N27 {median}, {len(comp['csize'])} components, min_points {k}")
        assert 0 < (comp["size"] < k).sum() < A.PPB


# ---- extremes --------------------------------------------------------------------------------------------------------------------
def test_moments_limit_reaches_the_headroom():
    xyz, bounds = oracle_rows("moments_limit")
    r = A.MOMENTS_R
    assert r == MC.MAX_RADIUS and MC.lattice_refusal(bounds, r) is None
    assert (1 << 31) <= 4 * r * r < (1 << 32) and (1 << 32) - 4 * r * r == 262140       # four squares fit 32 unsigned bits and not 31
    assert 2 * r * r >= 1 << 30                                                         # two mixed products of r * r would not fit 31 bits ...
    an = MC.analyse(xyz, r)
    special = np.nonzero((xyz != np.array(A.MOMENTS_FAR)).any(axis=1))[0]
    assert len(special) == 64 * len(A.MOMENTS_CLUSTERS) + 1 and len(np.unique(xyz // r, axis=0)) == 5
    # the definition over every pair of the special rows (the rest is copies of one point further than r from all of them)
    d = xyz[special][None, :, :] - xyz[special][:, None, :]
    d2 = (d * d).sum(axis=2)
    inside = d2 <= r * r
    assert np.array_equal(an["n"][special], inside.sum(axis=1)) and np.array_equal(an["s"][special], (d * inside[:, :, None]).sum(axis=1))
    assert np.array_equal(an["q"][special], np.stack([(d[:, :, a] * d[:, :, b] * inside).sum(axis=1) for a, b in MC.PRODUCTS], axis=1))
    far = np.setdiff1d(np.arange(A.PPB), special)
    assert (an["n"][far] == len(far)).all() and (an["s"][far] == 0).all() and (an["q"][far] == 0).all()
    assert np.abs(an["q"][:, (1, 2, 4)]).max() < 64 * r * r                             # ... but no pair here has two offsets of r
    at = lambda p: int(np.nonzero((xyz == np.array(p)).all(axis=1))[0][0])
    o, x, p = at((0, 0, 0)), at((r, 0, 0)), at(A.MOMENTS_OUTSIDE)
    k = list(special)
    got = dict(squares_at_limit=min(int((an["q"][:, c] >= 64 * r * r).sum()) for c in (0, 3, 5)),
               sums_at_limit=min(int((an["s"][:, c] <= -64 * r).sum()) for c in range(3)),
               one_outside=int(d2[k.index(o), k.index(p)] == r * r + 1 and not inside[k.index(o), k.index(p)] and d2[k.index(x), k.index(p)] == 1
                               and d2[k.index(o), k.index(x)] == r * r and inside[k.index(o), k.index(x)]))
    print(f"moments_limit: rows with q_xx, q_yy, q_zz >= 64 r^2: {[int((an['q'][:, c] >= 64 * r * r).sum()) for c in (0, 3, 5)]}, the largest {int(an['q'].max())}; "
          f"rows with s <= -64 r: {[int((an['s'][:, c] <= -64 * r).sum()) for c in range(3)]}; N of a row at the origin {int(an['n'][o])}, at (r, 0, 0) {int(an['n'][x])}, "
          f"at {A.MOMENTS_OUTSIDE} {int(an['n'][p])}; pairs_bound {an['pairs_bound']}")
    demand("moments_limit", got)


def test_neighbors_limit_reaches_the_radius():
    xyz, bounds = oracle_rows("neighbors_limit")
    r = A.NEIGHBORS_R
    assert r == NC.MAX_RADIUS and NC.lattice_refusal(bounds, r) is None
    pr = NC.properties(xyz, r)
    an = NC.analyse(xyz, r)
    nn2 = an["nn2"]
    real = nn2 != NC.NONE
    want = []
    for what, off, d2 in A.NEIGHBORS_PAIRS:
        inside = off is not None and d2 <= r * r
        want += [(2 if inside else 1, d2 if inside else None)] * (1 if off is None else 2)
    head = len(want)
    assert [(int(n), None if q == NC.NONE else int(q)) for n, q in zip(an["n"][:head], nn2[:head])] == want
    assert (an["n"][head:] == A.PPB - head).all() and (nn2[head:] == 0).all()
    got = dict(exactly_r=pr["exactly_r"], nn2_zero=pr["nn2_zero"], no_neighbour=pr["no_neighbour"], nn2_41_bits=int((real & (nn2 >= np.uint64(1 << 40))).sum()))
    print(f"neighbors_limit: {pr}; nn2 >= 2^40 on {got['nn2_41_bits']} rows, nn2 == 2^40 - 447 on {int((nn2 == np.uint64((1 << 40) - 447)).sum())}")
    assert pr["exactly_r"] >= 6 and int((nn2 == np.uint64((1 << 40) - 447)).sum()) == 2 and pr["no_neighbour"] >= 3
    demand("neighbors_limit", got)


# ---- shapes ----------------------------------------------------------------------------------------------------------------------
def test_shapes_are_deep_and_differ_by_connectivity():
    xyz, bounds = oracle_rows("shapes")
    plan = A.shapes_plan()
    vox = (0, 0, 0, A.SHAPES_CELL)
    assert K.lattice_refusal(bounds, vox) is None
    runs = K.count_runs(xyz, vox)
    assert runs == A.PPB and K.table_slots(runs) == 2 * A.PPB
    v = xyz // A.SHAPES_CELL
    rows_of = {}
    for name, voxels in plan.items():
        member = np.isin(A.keys_of(v), A.keys_of(voxels))
        rows_of[name] = np.nonzero(member)[0]
    assert sum(len(r) for r in rows_of.values()) == A.PPB
    sizes = {name: len(r) for name, r in rows_of.items()}
    assert len(plan["path"]) >= 8192 and sizes == dict(path=A.PPB - 2 * A.STAIRS, stairs=A.STAIRS, block=A.BLOCK ** 3 // 2)
    an26, an6 = K.analyse(xyz, vox, None, 26), K.analyse(xyz, vox, None, 6)
    assert sorted(an26["csize"].tolist()) == [A.STAIRS, A.STAIRS, sizes["path"]]
    assert sorted(an6["csize"].tolist()) == [1] * (2 * A.STAIRS) + [sizes["path"]]
    path_rows = xyz[rows_of["path"]]
    sweeps = K.sweeps(path_rows, vox, None, 6, 16)
    path = [tuple(p) for p in plan["path"].tolist()]
    ecc = {conn: A.graph_eccentricity(path, path[0], conn) for conn in (6, 26)}
    assert all(reached == len(path) for reached, _ in ecc.values())
    inside = 0
    for name in ("path", "stairs"):                                         # the least row of a structure does not lie at an end of it
        first = tuple(v[rows_of[name][0]].tolist())
        ends = (tuple(plan[name][0].tolist()), tuple(plan[name][-1].tolist()))
        inside += first not in ends
    print(f"shapes: {an26['voxels']} voxels; components {len(an26['csize'])} under 26, {len(an6['csize'])} under 6; rows {sizes}; the path: {len(path)} voxels, "
          f"{sweeps} neighbour-minimum sweeps (of at most 16) do not label it, its ends are {ecc[6][1]} (6) and {ecc[26][1]} (26) steps apart; "
          f"least rows: path {rows_of['path'][0]}, stairs {rows_of['stairs'][0]}, block {rows_of['block'][0]}")
    assert sweeps >= 12 and ecc[6][1] >= 8000 and ecc[26][1] >= 8000
    demand("shapes", dict(deep_path=min(ecc[6][1], ecc[26][1]) >= 8000, conn_differs=len(an6["csize"]) - len(an26["csize"]), least_row_inside=inside == 2))
