"""Numpy restatement of the flux fit by blend groups.  Two galaxies of a field are adjacent iff their
stamp rectangles, clipped to the field, intersect - the rectangle test of the dense fit's pair list; a stamp wholly outside its
field is adjacent to nothing, itself included.  A blend group is a connected component, found here with a plain union-find.
fit_group is the smallest row of the group counted from the field's first row, fit_group_size its members; the groups of a
field are ordered by fit_group and the members of a group stay in ascending row order.  The fit then is the dense restatement
(tests/fit_flux_oracle.py, tests/fit_flux_weighted_oracle.py - imported, not copied) on every group as if it were a field."""
import numpy as np

from tests import fit_flux_oracle as fo
from tests import fit_flux_weighted_oracle as fw


def adjacency(places, cs, F):
    """(n, n) bool: the clipped rectangles of rows i and j of ONE field intersect (the diagonal: the stamp touches the field)"""
    p = np.asarray(places, dtype=np.int64).reshape(-1, 2)
    lo = np.maximum(np.maximum(p[:, None, :], p[None, :, :]), 0)
    hi = np.minimum(np.minimum(p[:, None, :], p[None, :, :]) + cs, F)
    return (hi > lo).all(axis=2)


def components(adj):
    """(label, size) per row of one field from its adjacency matrix: union-find, the root the smallest row"""
    n = adj.shape[0]
    parent = np.arange(n)

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for i, j in zip(*np.nonzero(np.tril(adj, -1))):
        a, b = find(i), find(j)
        if a != b:
            parent[max(a, b)] = min(a, b)
    label = np.array([find(i) for i in range(n)], dtype=np.int32).reshape(n)
    size = np.bincount(label, minlength=n)[label].astype(np.int32) if n else np.zeros(0, np.int32)
    return label, size


def groups(places, field_ptr, cs, F):
    """fit_group and fit_group_size (N,) int32 of a call"""
    places = np.asarray(places, dtype=np.int64).reshape(-1, 2)
    fp = np.asarray(field_ptr, dtype=np.int64)
    group, size = np.zeros(len(places), np.int32), np.zeros(len(places), np.int32)
    for m in range(len(fp) - 1):
        lo, hi = int(fp[m]), int(fp[m + 1])
        group[lo:hi], size[lo:hi] = components(adjacency(places[lo:hi], cs, F))
    return group, size


def lists(places, field_ptr, cs, F):
    """The lists the host of the dense fit builds, in rows of the call: pairs (n_pairs, 2) of adjacent (i, j <= i) sorted by i
    and then j, and the CSR adjacency (adj_ptr (N + 1,), adj) with ascending lists"""
    places = np.asarray(places, dtype=np.int64).reshape(-1, 2)
    fp = np.asarray(field_ptr, dtype=np.int64)
    pairs, adj, ptr = [], [], [0]
    for m in range(len(fp) - 1):
        lo, hi = int(fp[m]), int(fp[m + 1])
        A = adjacency(places[lo:hi], cs, F)
        for i in range(hi - lo):
            js = np.nonzero(A[i])[0]
            pairs += [(lo + i, lo + j) for j in js if j <= i]
            adj += [lo + j for j in js]
            ptr.append(len(adj))
    return (np.array(pairs, np.int32).reshape(-1, 2), np.array(ptr, np.int32), np.array(adj, np.int32))


def group_order(group, field_ptr):
    """(order, group_ptr, field_of_group): the rows of the call in group order - the groups of a field by fit_group, the members
    ascending -, where every group begins in that order, and the field every group lies in"""
    fp = np.asarray(field_ptr, dtype=np.int64)
    order, gptr, gfield = [], [0], []
    for m in range(len(fp) - 1):
        lo, hi = int(fp[m]), int(fp[m + 1])
        g = np.asarray(group[lo:hi])
        for root in np.unique(g):
            order += (lo + np.nonzero(g == root)[0]).tolist()
            gptr.append(len(order))
            gfield.append(m)
    return np.array(order, np.int64), np.array(gptr, np.int64), np.array(gfield, np.int64)


def serpentine(n, cs, F):
    """n placements inside a field of F pixels along a serpentine path whose consecutive stamps overlap by one pixel: lines 2 (cs
    - 1) apart, joined at alternating ends by one stamp half way between them - one long chain for the labels to cross"""
    step = cs - 1
    per = (F - cs) // step + 1
    path, y, fwd = [], 0, True
    while len(path) < n:
        xs = [i * step for i in range(per)]
        xs = xs if fwd else xs[::-1]
        path += [(y, x) for x in xs]
        path.append((y + step, xs[-1]))
        y, fwd = y + 2 * step, not fwd
    path = np.array(path[:n], np.int32)
    assert (path >= 0).all() and (path + cs <= F).all()
    return path


def fit_flux_groups(stamps, places, field_ptr, data_fields, weight_fields=None, min_pivot=1e-8):
    """The outputs of dv_scene_fit_flux_groups: the dense restatement on every blend group as if it were a field (the data and
    weight fields of a group are those of its field, by reference), scattered back to the rows of the call, plus fit_group and
    fit_group_size.  Returns (out, groups) with groups[g] the dense restatement's per-field dictionary of group g."""
    stamps = np.asarray(stamps, dtype=np.float32)
    places = np.asarray(places, dtype=np.int64).reshape(-1, 2)
    cs, F = stamps.shape[1], np.asarray(data_fields[0]).shape[0]
    group, size = groups(places, field_ptr, cs, F)
    order, gptr, gfield = group_order(group, field_ptr)
    D = [data_fields[m] for m in gfield]
    if weight_fields is None:
        sub, per_group = fo.fit_flux(stamps[order], places[order], gptr, D, min_pivot)
    else:
        sub, per_group = fw.fit_flux(stamps[order], places[order], gptr, D, [weight_fields[m] for m in gfield], min_pivot)
    out = {}
    for k, a in sub.items():
        out[k] = np.zeros_like(a)
        out[k][order] = a
    out["fit_group"], out["fit_group_size"] = group, size
    return out, per_group
