"""Painted fields for the detector's segmentation and deblender ("Tests"): fields that are exactly 0
outside shapes painted with small integers, aimed at one piece of csrc/detect.hip each, and the premises under which the
comparison with the numpy restatement is exact.  numpy and scipy only.

The regime.  In a field that is 0 outside the shapes every background mesh has median 0, the median-filtered mesh grid is
0 and a spline through zeros is 0: back == 0 and v == data.  With filter_kernel [[1.0]] D == v bit for bit.  On the weighted
path with unit weights, noise "absolute", filter_type "conv" and thresh 0.5 the threshold is 0.5 exactly, so segmentation
and deblender see the painted integers.  The unweighted path reaches the same regime where 1.5 * globalrms falls strictly
between 0 and the smallest painted value (UNWEIGHTED names the cases; tests/test_detect_shapes_host.py asserts the list).

Every builder returns (data, kwargs, facts): the field, the settings that both paths share (minarea, cont) and the
structure the case exists for.  check_premises asserts P1 - P4 on the oracle's output, check_facts P5."""
import functools

import numpy as np
import scipy.ndimage

from tests import detect_oracle as do
from tests import detect_weighted_oracle as wo

H, W = 125, 157                  # H != W, neither a multiple of 16 or 64: partial meshes, filter tiles and last block
K1 = np.array([[1.0]])
EIGHT = np.ones((3, 3), dtype=bool)


def weighted_kwargs(kw):
    return dict(noise="absolute", filter_type="conv", thresh=0.5, filter_kernel=K1, **kw)


def unweighted_kwargs(kw):
    return dict(thresh=1.5, filter_kernel=K1, **kw)


# ---- the painted fields -----------------------------------------------------------------------------------------------
def row_wrap():
    """bars that end at column W - 1 next to bars that start at column 0 in the same row, one row below and two rows below
    (the raster neighbours p - 1, p - W + 1 and p - W - 1 of a pixel at the field's edge), single pixels in the two far
    corners, and one component that holds both ends of six rows: two blocks on a full row, which the level loop must keep
    apart.  Aimed at the c > 0 and c + 1 < W guards of cc_merge_kernel and of the level loop of deblend_kernel."""
    d = np.zeros((H, W))
    n = 0
    for i, r in enumerate(range(2, 100, 4)):
        d[r, W - 2 - i % 3:] = 2 + i % 2
        d[r + (1, 0, 2)[i % 3], :2 + (i + 1) % 3] = 3 - i % 2
        n += 2
    d[0, 0] = 2
    d[H - 1, W - 1] = 3
    d[112, :] = 1
    d[106:112, :40] = 5
    d[106:112, W - 30:] = 3
    return d, dict(minarea=1), dict(components=n + 3, objects=n + 4, objects_per_component={106 * W: 2})


def diagonals():
    """an anti-diagonal and a main-diagonal staircase of single pixels, 85 px each, connected through q + 1 and q - 1
    alone; the anti-diagonal ends three rows above the point where it would meet the other"""
    d = np.zeros((H, W))
    i = np.arange(85)
    d[2 + i, 150 - i] = 4
    d[30 + i, 4 + i] = 3
    return d, dict(), dict(components=2, objects=2, labels={2 * W + 150: 85, 30 * W + 4: 85})


def _serpentine(r0, nrows, c0, width, value):
    d = np.zeros((H, W))
    for i in range(nrows):
        r = r0 + 4 * i
        d[r, c0:c0 + width] = value
        if i + 1 < nrows:
            d[r + 1:r + 4, c0 + width - 1 if i % 2 == 0 else c0] = value
    return d


def serpentine():
    """a full row every fourth row, joined alternately at the right and the left end: one component of 5117 px (the
    global-scratch path) whose bounding box is the field.  Aimed at uf_union's retry path under long chains across many
    workgroups, at cc_flatten's box atomics and at a bounding-box scan far larger than n."""
    d = _serpentine(0, 32, 0, W, 1.0)
    n = int((d > 0).sum())
    return d, dict(), dict(components=1, objects=1, labels={0: n}, npix=[n], above_lds=True)


def spiral():
    """a square spiral with arm spacing 4: one component of 3841 px in a 121 x 121 box"""
    d = np.zeros((H, W))
    r, c = 2, 3
    d[r, c] = 2
    lens = [120, 120, 120]
    for side in range(116, 0, -4):
        lens += [side, side]
    for k, side in enumerate(lens):
        dr, dc = ((0, 1), (1, 0), (0, -1), (-1, 0))[k % 4]
        for _ in range(side):
            r, c = r + dr, c + dc
            d[r, c] = 2
    n = int((d > 0).sum())
    return d, dict(), dict(components=1, objects=1, labels={2 * W + 3: n}, npix=[n], above_lds=True)


def half_serpentine():
    """the serpentine at half size (1645 px: the LDS path) with three of its U-turns raised to 5, 7 and 4: the level loop
    runs its union-finds along the winding core for every level below 1 and splits it into three objects above"""
    r0, c0, width = 1, 2, 100
    d = _serpentine(r0, 16, c0, width, 1.0)
    for turn, value in ((2, 5.0), (7, 7.0), (12, 4.0)):
        r = r0 + 4 * turn
        cols = slice(c0 + width - 8, c0 + width) if turn % 2 == 0 else slice(c0, c0 + 8)
        d[r:r + 5, cols] = np.where(d[r:r + 5, cols] > 0, value, 0.0)
    n = int((d > 0).sum())
    assert n <= 2048
    return d, dict(), dict(components=1, objects=3, labels={r0 * W + c0: n}, above_lds=False)


def _lattice():
    d = np.zeros((H, W))
    rr, cc = np.meshgrid(np.arange(1, H, 2), np.arange(19, 65, 2), indexing="ij")
    # two values, 18 % of two meshes: a third value or fewer columns and the clipping empties every mesh (globalrms 0)
    d[rr, cc] = 3 + (rr // 2 + cc // 2) % 2
    return d


def lattice():
    """1426 single pixels of 3 and 4 on every second row and column, rows 1 to 123, minarea 1: one object per pixel in
    raster order.  Aimed at the cc_compact scan across 4096-pixel blocks (five of them, up to 8 hits per thread), the host's
    slot and scratch placement for more than a thousand jobs and cap = n for minarea 1."""
    d = _lattice()
    n = int((d > 0).sum())
    assert 1000 <= n <= 1500
    return d, dict(minarea=1), dict(components=n, objects=n, raster=True)


def lattice_minarea2():
    """the lattice with minarea 2: no component is kept"""
    return _lattice(), dict(minarea=2), dict(components=0, objects=0)


def _comb():
    d = np.zeros((H, W))
    d[100, 3:153] = 1
    for i in range(25):
        c = 3 + 6 * i
        d[70:100, c:c + 3] = 1
        top = 72 if i % 2 == 0 else 75
        d[top:top + 6, c:c + 3] = 4 + i % 3
        if i % 2 == 0:
            d[top + 5, c + 2] += 1               # the peak at the end of the bump that starts first ...
        else:
            d[top, c] += 1                       # ... and at the start of the bump that starts later
    return d


def comb():
    """a one-pixel backbone with 25 teeth, each with a bump of 4, 5 or 6 and a peak pixel one above it.  The even teeth's
    bumps start three rows above the odd ones' and have their peak in their last row: the object list (nodes in raster
    order) and the catalogue (peak pixels) are in different orders.  Aimed at the serial decision rule, chid, ostate, othr2
    and the insertion sort."""
    return _comb(), dict(), dict(components=1, objects=25, reordered=True)


def comb_minarea1():
    return _comb(), dict(minarea=1), dict(components=1, objects=25, reordered=True)


def nested_mesas():
    """a base of 1, two mesas of 3 on it, two towers of 7 on each mesa: 1 -> 2 -> 4 objects at two levels.  Aimed at the
    renumbering after a second split, where obj is already non-zero."""
    d = np.zeros((H, W))
    d[20:60, 20:120] = 1
    d[24:56, 24:64] = 3
    d[24:56, 76:116] = 3
    d[30:50, 28:40] = 7
    d[28:46, 48:58] = 7
    d[32:52, 80:90] = 7
    d[30:44, 100:112] = 7
    return d, dict(), dict(components=1, objects=4, nobj_log=[1, 2, 4])


def insignificant():
    """two components that stay one object each: in the first the second mesa's flux (18) is below cont * flux(component)
    (0.2 * 1212), in the second the second mesa has minarea - 1 = 3 pixels, of a flux (21) above 0.2 * 68.  A third, the
    control, has two mesas of 300 and 360 on a component of 940 and splits in two.  Aimed at the nflux > cont * cflux
    filter, the cnt >= minarea node filter and the count of significant nodes that splits an object (two)."""
    d = np.zeros((H, W))
    d[10:30, 10:50] = 1
    d[14:24, 14:24] = 5
    d[14:16, 40:43] = 3
    d[60:63, 60:70] = 1
    d[61, 61:65] = 6
    d[61, 66:69] = 7
    d[90:100, 20:60] = 1
    d[92:98, 24:34] = 5
    d[92:98, 44:54] = 6
    return d, dict(cont=0.2), dict(components=3, objects=4, branches=[2, 2, 2], splits=[0, 0, 1])


def plateaus():
    """three flat-topped objects on one base.  The plateau of the second starts two rows below and forty columns left of
    the first's, which is 1107 px large.  Aimed at the smallest-index rule of blk_argmax and the order by peak pixel."""
    d = np.zeros((H, W))
    d[10:51, 10:111] = 1
    d[14:41, 60:101] = 5
    d[16:20, 20:28] = 4
    d[30:46, 30:41] = 6
    return d, dict(), dict(components=1, objects=3, peak_pixels=[14 * W + 60, 16 * W + 20, 30 * W + 30], peaks=[5, 4, 6])


def zero():
    return np.zeros((H, W)), dict(minarea=1), dict(components=0, objects=0)


def first_row():
    d = np.zeros((H, W))
    d[0, :] = 2
    return d, dict(minarea=1), dict(components=1, objects=1, labels={0: W})


def last_row():
    d = np.zeros((H, W))
    d[H - 1, :] = 2
    return d, dict(minarea=1), dict(components=1, objects=1, labels={(H - 1) * W: W})


CASES = dict(row_wrap=row_wrap, diagonals=diagonals, serpentine=serpentine, spiral=spiral, half_serpentine=half_serpentine,
             lattice=lattice, lattice_minarea2=lattice_minarea2, comb=comb, nested_mesas=nested_mesas,
             insignificant=insignificant, plateaus=plateaus, comb_minarea1=comb_minarea1, zero=zero, first_row=first_row,
             last_row=last_row)
# the fields of the batch (one call, minarea 1): more than a thousand components next to none, painted first and last rows
BATCH = ("lattice", "zero", "last_row", "first_row", "comb_minarea1")
# band 2 of the two fields of the band-gather case, and the painted decoys of the other bands
BANDS = ("nested_mesas", "comb")
DECOYS = ("diagonals", "plateaus", "insignificant", "half_serpentine", "spiral")
# the cases in which 0 < 1.5 * globalrms < 0.9 * (smallest painted value): the unweighted path sees the painted integers
UNWEIGHTED = ("serpentine", "spiral", "half_serpentine", "lattice", "lattice_minarea2", "comb", "nested_mesas", "plateaus",
              "comb_minarea1")


# ---- the oracle's answer and the premises -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle(name, path="weighted"):
    """(data, oracle result, per-component details, kwargs of the path) of a case; computed once, treat as read-only"""
    data, kw, _ = CASES[name]()
    details = []
    if path == "weighted":
        kw = weighted_kwargs(kw)
        exp = wo.detect(data, np.ones_like(data), details=details, **kw)
    else:
        kw = unweighted_kwargs(kw)
        exp = do.detect(data, details=details, **kw)
    for a in [data] + [v for v in exp.values() if isinstance(v, np.ndarray)]:
        a.setflags(write=False)
    return data, exp, details, kw


def threshold(exp, kw):
    return kw["thresh"] if kw.get("noise") == "absolute" else kw["thresh"] * exp["globalrms"]


def unweighted_premise(data, exp):
    """0 < 1.5 * globalrms < 0.9 * (smallest painted value)"""
    painted = data[data > 0]
    return len(painted) > 0 and 0.0 < 1.5 * exp["globalrms"] < 0.9 * painted.min()


def check_premises(data, exp, details, kw, back_size=64):
    """P1 - P4: conditions on the input, asserted on the oracle's output alone"""
    # P1: the background is exactly 0 and D is the data bit for bit
    assert (exp["back"] == 0.0).all(), "P1: back"
    assert np.array_equal(exp["D"], data) and not np.signbit(exp["D"][data == 0]).any(), "P1: D"
    # P2: no mesh is within 1e-9 of the switch between 2.5 med - 1.5 mean and med.  A kept set of zeros alone is exempt:
    # its mean and sigma are sums of zeros, 0 in every summation order, and both branches give 0.
    for i in range(0, data.shape[0], back_size):
        for j in range(0, data.shape[1], back_size):
            m = {}
            do.mesh_stats(data[i:i + back_size, j:j + back_size], details=m)
            if not (m["kept"] == 0.0).all():
                assert abs(abs(m["mean"] - m["med"]) - 0.3 * m["sig"]) >= 1e-9, ("P2", i, j)
    T = threshold(exp, kw)
    for c in details:
        assert c["T"] == T
        # P3: no pixel value of the component within 1e-6 P of a level it reaches
        vals = np.unique(c["values"])
        gap = np.abs(vals[:, None] - np.asarray(c["levels"])[None, :]).min() if len(c["levels"]) else np.inf
        assert gap >= 1e-6 * vals.max(), ("P3", int(c["pix"][0]), gap)
        # P4: every pixel assigned by score has a best score 1e-6 (relative) above the second best
        if c["score"] is not None and c["free"].any():
            s = np.sort(c["score"][:, c["free"]], axis=0)
            assert (s[-1] > 0.0).all() and (s[-1] - s[-2] >= 1e-6 * s[-1]).all(), ("P4", int(c["pix"][0]))


def scipy_labels(data, T, minarea):
    """the label map from scipy.ndimage.label alone: 8-connected components of data > T named by their first raster index,
    those of fewer than minarea pixels -1"""
    lab, n = scipy.ndimage.label(data > T, structure=EIGHT)
    flat = lab.ravel()
    out = np.full(flat.shape, -1, dtype=np.int64)
    if n:
        idx = np.arange(flat.size)
        first = scipy.ndimage.minimum(idx, labels=flat, index=np.arange(1, n + 1)).astype(np.int64)
        area = np.bincount(flat, minlength=n + 1)[1:]
        on = flat > 0
        keep = area[flat[on] - 1] >= minarea
        out[idx[on][keep]] = first[flat[on] - 1][keep]
    return out.reshape(data.shape)


def check_facts(data, exp, details, facts):
    """P5: the structure the case exists for"""
    Wd = data.shape[1]
    parents = np.unique(exp["parent"])
    assert len(parents) == len(details) == facts["components"], (len(parents), facts["components"])
    assert len(exp["x"]) == facts["objects"], (len(exp["x"]), facts["objects"])
    if facts["components"] == 0:
        assert (exp["labels"] == -1).all()
    for root, n in facts.get("labels", {}).items():
        assert (exp["labels"] == root).sum() == n and exp["labels"].ravel()[root] == root, root
        assert root == np.flatnonzero(exp["labels"].ravel() == root)[0]
    for root, n in facts.get("objects_per_component", {}).items():
        assert (exp["parent"] == root).sum() == n, root
    if "npix" in facts:
        assert exp["npix"].tolist() == facts["npix"] == [int((data > 0).sum())]
    if "above_lds" in facts:                                   # which side of the deblend kernel's LDS budget (2048 px)
        c = details[0]
        assert (len(c["pix"]) > 2048) == facts["above_lds"]
        if facts["above_lds"]:                                 # the scan of the bounding box is far larger than n
            r, col = c["pix"] // Wd, c["pix"] % Wd
            assert (np.ptp(r) + 1) * (np.ptp(col) + 1) > 3 * len(c["pix"])
    if facts.get("raster"):                                    # one object per painted pixel, in raster order
        painted = np.flatnonzero(data.ravel() > 0)
        assert np.array_equal(exp["parent"], painted) and (exp["npix"] == 1).all()
        assert np.array_equal(exp["peak"], data.ravel()[painted])
    if facts.get("reordered"):                                 # the object list is not in the catalogue's order
        c = details[0]
        assert len(c["split_levels"]) == 1 and (np.diff(c["core_first"]) > 0).all()
        order = np.argsort(c["peak_pixels"])
        assert (np.diff(c["peak_pixels"]) < 0).sum() >= 1 and (order != np.arange(len(order))).sum() >= 20
    if "nobj_log" in facts:                                    # the object list's length, level by level
        c = details[0]
        log = [n for n, prev in zip(c["nobj"], [0] + c["nobj"][:-1]) if n != prev]
        assert log == facts["nobj_log"] and len(c["split_levels"]) == len(log) - 1, (log, c["split_levels"])
    if "branches" in facts:                                    # what the filters turn down would have been a second node
        for c, n, splits in zip(details, facts["branches"], facts["splits"]):
            m = np.zeros(data.shape, dtype=bool)
            m.ravel()[c["pix"]] = c["values"] > 1
            assert scipy.ndimage.label(m, structure=EIGHT)[1] == n
            assert len(c["split_levels"]) == splits and len(c["peak_pixels"]) == 1 + splits
    if "peak_pixels" in facts:                                 # every peak pixel is the first pixel of its plateau
        c = details[0]
        assert sorted(c["peak_pixels"]) == facts["peak_pixels"]
        assert exp["peak"].tolist() == facts["peaks"]
        for o, pk in enumerate(c["peak_pixels"]):
            p = c["pix"][c["assign"] == o]
            top = p[data.ravel()[p] == data.ravel()[p].max()]
            assert len(top) > 30 and top.min() == pk
