"""Cases and the numpy side of the connected-component tests (tests/test_components_cpu.py checks on the CPU, against the oracle's
decoder, that the cases do what tests/test_gpu_components.py needs them to do). The streams, clips and lattices are those of
tests/thin_cases.py and tests/denoise_cases.py. Inputs and reference arithmetic only."""
from __future__ import annotations

import numpy as np

from tests import denoise_cases as D
from tests import thin_cases as T

PPB = T.PPB
KEEP, SMALL = 0, 1                                  # PCR_COMPONENTS_KEEP / PCR_COMPONENTS_SMALL
KEY_BITS = T.KEY_BITS
HUGE = 1 << 40                                      # a min_points no component reaches: everything is small
STREAMS, ORIGINS, COMBOS, WIDE30_LOW = T.STREAMS, T.ORIGINS, D.COMBOS, T.WIDE30_LOW
stream, clip_for, case_clip, xyz_of, candidates = T.stream, T.clip_for, T.case_clip, T.xyz_of, T.candidates
count_runs, decoded_batches, table_slots, lattice_refusal = T.count_runs, T.decoded_batches, T.table_slots, D.lattice_refusal

# The preconditioned cases: (stream, cell, connectivity, clip -- None, "stream" for clip_for()'s, or a box -- , min_points, what the
# oracle's decode gave: voxels, components, the largest sizes, components with candidates in two or more batches), origin (0, 0, 0),
# and the properties each shows (see properties()).
CASES = [
    ("clustered", 1000, 26, None, 1000, (21963, 202, (87982, 59976, 59951, 59789), 3), ("both_classes", "multi_batch", "deep", "conn_differs")),
    ("clustered", 1000, 6, None, 1000, (21963, 870, (87778, 59847), 6), ("both_classes", "multi_batch", "deep", "conn_differs")),
    ("synth", 1000, 26, None, 13, (599887, 31715, (55368, 98, 74, 63), 1033), ("both_classes", "multi_batch", "many")),
    ("synth", 2048, 26, "stream", 2000, (56738, 21, (115364, 2247, 1890, 1476), 4), ("both_classes", "multi_batch", "deep")),
    ("garbage_tail", 2048, 6, "stream", 25, (249632, 127, (327346, 24, 13, 10), 2), ("both_classes", "multi_batch", "deep")),
    ("wide30", 1, 26, WIDE30_LOW, 6000, (58942, 2096, (13539, 7205, 6341, 6097), 794), ("both_classes", "multi_batch", "deep", "many")),
    ("escape_heavy", 7001, 26, None, 26, (120362, 9761, (116599, 25, 21, 17), 25), ("both_classes", "multi_batch", "deep", "many")),
    ("plateau", 64, 26, None, 20, (122754, 70364, (23, 20, 20, 19), 53), ("both_classes", "multi_batch", "many")),
]
# plain neighbour-minimum sweeps to the fixed point, as measured when the cases were chosen: `deep` is sweeps >= 32
SWEEPS = [46, 62, 21, 301, 1052, 284, 331, 16]
PROPERTIES = ("both_classes", "multi_batch", "deep", "conn_differs", "many")


def forward_offsets(connectivity: int):
    """Half of the neighbourhood as key differences: every undirected edge once."""
    assert connectivity in (6, 26)
    out = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dz, dy, dx) <= (0, 0, 0) or (connectivity == 6 and abs(dx) + abs(dy) + abs(dz) != 1):
                    continue
                out.append(dx + dy * (1 << KEY_BITS) + dz * (1 << (2 * KEY_BITS)))
    assert len(out) == (13 if connectivity == 26 else 3)
    return out


def label_graph(n: int, u, v):
    """Per node 0 .. n - 1 of the undirected graph with edges (u[k], v[k]) the least node of its component: hooking by minimum
    and pointer jumping, a logarithmic number of rounds instead of one per step of the diameter."""
    p = np.arange(n, dtype=np.int64)
    u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
    while len(u):
        pu, pv = p[u], p[v]
        open_ = pu != pv
        u, v, pu, pv = u[open_], v[open_], pu[open_], pv[open_]
        if len(u) == 0:
            break
        m = np.minimum(pu, pv)
        np.minimum.at(p, pu, m)                     # the greater root goes under the lesser one (p[i] <= i throughout)
        np.minimum.at(p, pv, m)
        while True:                                 # every node to its root
            q = p[p]
            if np.array_equal(q, p):
                break
            p = q
    return p


def analyse(xyz, vox, clip=None, connectivity=26):
    """What a components call over the rows `xyz` (int [n, 3], in row order) finds, whatever min_points: a dict of
      rows    the candidates' rows, int64, increasing
      label   per candidate: the least row of its component
      size    per candidate: the candidates of its component
      voxels  the non-empty voxels
      clabel / csize  per component: its label (increasing) and its size
    Keys as tests/denoise_cases.py's analyse (np.unique with counts and first occurrences), edges by searchsorted of the shifted
    keys, labels by label_graph over the voxels ranked by their least row."""
    m = candidates(xyz, clip)
    rows = np.nonzero(m)[0].astype(np.int64)
    empty = np.zeros(0, np.int64)
    if len(rows) == 0:
        return dict(rows=rows, label=empty, size=empty, voxels=0, clabel=empty, csize=empty)
    org, cell = np.array(vox[:3], np.int64), int(vox[3])
    v = np.floor_divide(np.asarray(xyz, np.int64)[m] - org, cell)
    v = v - v.min(axis=0) + 1
    assert int(v.max()) + 1 < 1 << KEY_BITS, "the voxels of the candidates do not fit the key"
    key = v[:, 0] | (v[:, 1] << KEY_BITS) | (v[:, 2] << (2 * KEY_BITS))
    uniq, first, inv, count = np.unique(key, return_index=True, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    least = rows[first]                             # per voxel its least row: np.unique's first occurrence
    rank = np.empty(len(uniq), np.int64)            # voxel -> its position by least row
    order = np.argsort(least)
    rank[order] = np.arange(len(uniq))
    eu, ev = [], []
    for off in forward_offsets(connectivity):
        other = uniq + off
        at = np.minimum(np.searchsorted(uniq, other), len(uniq) - 1)
        hit = uniq[at] == other
        eu.append(rank[np.nonzero(hit)[0]])
        ev.append(rank[at[hit]])
    root = label_graph(len(uniq), np.concatenate(eu), np.concatenate(ev))       # over ranks: the least rank is the least row
    vlabel = least[order][root][rank]               # per voxel, in uniq's order
    clabel, cinv = np.unique(vlabel, return_inverse=True)
    csize = np.bincount(cinv.reshape(-1), weights=count, minlength=len(clabel)).astype(np.int64)
    vsize = csize[cinv.reshape(-1)]
    return dict(rows=rows, label=vlabel[inv], size=vsize[inv], voxels=len(uniq), clabel=clabel, csize=csize)


def select(an, min_points: int, mode: int = KEEP):
    """(rows, labels) pcr_components writes, from analyse()'s dict: a component is small iff its size < min_points."""
    small = an["size"] < min_points
    pick = small if mode == SMALL else ~small
    return an["rows"][pick], an["label"][pick]


def reference(xyz, vox, min_points, clip=None, connectivity=26, mode=KEEP):
    return select(analyse(xyz, vox, clip, connectivity), min_points, mode)


def stats(an, min_points: int):
    """The fields of pcr_components_stats the components decide."""
    small = an["csize"] < min_points
    return dict(voxels=int(an["voxels"]), components=len(an["csize"]), components_small=int(small.sum()), points_small=int(an["csize"][small].sum()),
                largest_points=int(an["csize"].max()) if len(an["csize"]) else 0)


def median_size(an) -> int:
    """The median of the component size over the candidates (the upper one of an even number): an exact integer; 0 without
    candidates."""
    n = an["size"]
    return int(np.sort(n)[len(n) // 2]) if len(n) else 0


def sweeps(xyz, vox, clip=None, connectivity=26, limit=40):
    """Plain neighbour-minimum sweeps over the voxels until one changes nothing, that one counted, at most `limit`: the count,
    or `limit` if the labels still change then (the diameter of a component in voxels is a lower bound of what a fixed number of
    rounds needs)."""
    m = candidates(xyz, clip)
    org, cell = np.array(vox[:3], np.int64), int(vox[3])
    v = np.floor_divide(np.asarray(xyz, np.int64)[m] - org, cell)
    v = v - v.min(axis=0) + 1
    key = v[:, 0] | (v[:, 1] << KEY_BITS) | (v[:, 2] << (2 * KEY_BITS))
    uniq, first = np.unique(key, return_index=True)
    lab = first.astype(np.int64)
    pairs = []
    for off in forward_offsets(connectivity):
        other = uniq + off
        at = np.minimum(np.searchsorted(uniq, other), len(uniq) - 1)
        hit = np.nonzero(uniq[at] == other)[0]
        pairs.append((hit, at[hit]))
    for k in range(limit):
        new = lab.copy()
        for a, b in pairs:
            mn = np.minimum(lab[a], lab[b])
            np.minimum.at(new, a, mn)
            np.minimum.at(new, b, mn)
        if np.array_equal(new, lab):
            return k + 1
        lab = new
    return limit


def properties(xyz, vox, min_points, clip=None, connectivity=26):
    """What tests/test_components_cpu.py asserts, over the rows `xyz` of a whole stream:
      voxels / components / largest (the four largest sizes, decreasing)
      kept / small     candidates of either class at min_points
      multi_batch      components with candidates in two or more batches: the label has to cross workgroups
      sweeps           sweeps(..., limit=32): 32 or more sweeps are needed, so no fixed small number of rounds labels it
      conn_differs     the other connectivity gives another partition"""
    an = analyse(xyz, vox, clip, connectivity)
    small = an["size"] < min_points
    batch = an["rows"] >> 16
    _, comp = np.unique(an["label"], return_inverse=True)
    comp = comp.reshape(-1)
    lo = np.full(len(an["clabel"]), np.iinfo(np.int64).max)
    hi = np.full(len(an["clabel"]), -1)
    np.minimum.at(lo, comp, batch)
    np.maximum.at(hi, comp, batch)
    other = analyse(xyz, vox, clip, 6 if connectivity == 26 else 26)
    return dict(voxels=an["voxels"], components=len(an["csize"]), largest=tuple(int(s) for s in np.sort(an["csize"])[::-1][:4]),
                kept=int((~small).sum()), small=int(small.sum()), multi_batch=int((hi > lo).sum()), sweeps=sweeps(xyz, vox, clip, connectivity, 32),
                conn_differs=not np.array_equal(other["label"], an["label"]))
