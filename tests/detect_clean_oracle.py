"""numpy restatement of the detector's cleaning pass, after SExtractor's clean.c / sep's clean().
numpy only.

It works on what tests/detect_objects_oracle.py gives for one field - the raw objects' columns, npix and the segmap - plus
the catalogue columns of the detector restatement, the thresholded map D and the field's threshold T.  The rule, per field,
with beta = clean_param:

  det = x2 y2 - xy xy, area = pi sqrt(det), cxx = y2 / det, cyy = x2 / det, cxy = -2 xy / det,
  a = sqrt((x2 + y2) / 2 + sqrt(((x2 - y2) / 2)^2 + xy^2)), amp = dflux / (2 area),
  alpha = (pow(amp / T, 1 / beta) - 1) area / npix,
  mthresh = the minarea-th largest D - T over the object's pixels (0 with fewer than minarea pixels).

j is a candidate to absorb i iff j != i, dflux_j > dflux_i (or equal and j < i), T > 0, dx dx + dy dy < 100 (a_i + a_j)^2
with dx = x_iso_i - x_iso_j, dy = y_iso_i - y_iso_j, and P > mthresh_i, where
val = 1 + alpha_j ((cxx_j dx) dx + (cyy_j dy) dy + (cxy_j dx) dy) and P = amp_j pow(val, -beta) if 1 < val < 1e10, else 0.
absorber[i] is the candidate of the largest P (ties to the smaller row), i itself without one; every object goes to the root
of its chain; every test reads the raw values.  The merged row follows sep's mergeobject."""
import numpy as np

from tests import detect_objects_oracle as oo

PI = 3.141592653589793
MERGED = 16
CAT_KEYS = ("npix", "peak", "flux", "x", "y", "parent")
SHARED = CAT_KEYS + oo.INT_KEYS + oo.DOUBLE_KEYS           # the columns the cleaned rows share with the raw ones


def mthresh(segmap, D, T, n, minarea):
    """per raw object k (segmap number k + 1): the minarea-th largest D - T of its pixels, 0.0 with fewer"""
    out = np.zeros(n, dtype=np.float64)
    seg, Df = segmap.ravel(), D.ravel()
    order = np.argsort(seg, kind="stable")
    cuts = np.searchsorted(seg[order], np.arange(1, n + 2))
    for k in range(n):
        d = Df[order[cuts[k]:cuts[k + 1]]] - T
        if len(d) >= minarea:
            out[k] = np.sort(d)[len(d) - minarea]
    return out


def profile(obj, T, beta):
    """per raw object: a, amp, alpha, cxx, cyy, cxy"""
    x2, y2, xy = obj["x2"], obj["y2"], obj["xy"]
    with np.errstate(all="ignore"):
        det = x2 * y2 - xy * xy
        area = PI * np.sqrt(det)
        hd = (x2 - y2) / 2.0
        amp = obj["dflux"] / (2.0 * area)
        return dict(a=np.sqrt((x2 + y2) / 2.0 + np.sqrt(hd * hd + xy * xy)), amp=amp,
                    alpha=(np.power(amp / T, 1.0 / beta) - 1.0) * area / obj["npix"].astype(np.float64),
                    cxx=y2 / det, cyy=x2 / det, cxy=-2.0 * xy / det)


def pairs(obj, mth, T, beta):
    """the n x n tables of the pair test, [i, j] = (j absorbs i): zone (the pair can form), val, P and cand"""
    n = len(mth)
    pr = profile(obj, T, beta)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    df = obj["dflux"]
    with np.errstate(all="ignore"):
        brighter = (df[None, :] > df[:, None]) | ((df[None, :] == df[:, None]) & (j < i))
        dx = obj["x_iso"][:, None] - obj["x_iso"][None, :]
        dy = obj["y_iso"][:, None] - obj["y_iso"][None, :]
        sa = pr["a"][:, None] + pr["a"][None, :]
        zone = (i != j) & brighter & (T > 0) & (dx * dx + dy * dy < 100.0 * (sa * sa))
        val = 1.0 + pr["alpha"][None, :] * ((pr["cxx"][None, :] * dx) * dx + (pr["cyy"][None, :] * dy) * dy
                                            + (pr["cxy"][None, :] * dx) * dy)
        inside = (val > 1.0) & (val < 1e10)
        P = np.where(inside, pr["amp"][None, :] * np.power(np.where(inside, val, 2.0), -beta), 0.0)
        cand = zone & (P > mth[:, None])
    return dict(zone=zone, val=val, P=P, cand=cand, profile=pr)


def clean(cat, obj, D, T, minarea=4, clean_param=1.0):
    """One field.  cat: the catalogue columns CAT_KEYS of the detector restatement; obj: the result of
    detect_objects_oracle.objects (columns, npix, segmap); D, T: the thresholded map and the field's threshold.  Returns a
    dict: the cleaned columns (SHARED, nmerged, mthresh), segmap, n_raw, and for the premises and the tests absorber, root,
    survivors (raw rows), mthresh_raw and the tables of pairs()."""
    n = len(obj["npix"])
    raw = {k: np.asarray(cat[k]) for k in CAT_KEYS}
    raw.update({k: np.asarray(obj[k]) for k in oo.INT_KEYS + oo.DOUBLE_KEYS})
    assert np.array_equal(raw["npix"], obj["npix"])
    mth = mthresh(obj["segmap"], D, T, n, minarea)
    tab = pairs(obj, mth, T, clean_param)
    absorber = np.arange(n)
    for i in range(n):
        js = np.flatnonzero(tab["cand"][i])
        if len(js):
            absorber[i] = js[np.argmax(tab["P"][i, js])]        # the first maximum: the smaller row
    root = absorber.copy()
    while not np.array_equal(root[root], root):
        root = root[root]
    survivors = np.flatnonzero(root == np.arange(n))
    newrow = np.full(n, -1, dtype=np.int64)
    newrow[survivors] = np.arange(len(survivors))
    out = {k: raw[k][survivors].copy() for k in SHARED}
    out["nmerged"] = np.ones(len(survivors), dtype=np.int32)
    out["mthresh"] = mth[survivors].copy()
    peak_from = survivors.copy()                                # the raw row the merged peak / vpeak come from
    vpeak_from = survivors.copy()
    flux_terms = [[raw["flux"][s]] for s in survivors]
    dflux_terms = [[raw["dflux"][s]] for s in survivors]
    for r in range(n):                                          # the victims in ascending raw row
        if root[r] == r:
            continue
        k = newrow[root[r]]
        out["npix"][k] += raw["npix"][r]
        out["flux"][k] = out["flux"][k] + raw["flux"][r]
        out["dflux"][k] = out["dflux"][k] + raw["dflux"][r]
        flux_terms[k].append(raw["flux"][r])
        dflux_terms[k].append(raw["dflux"][r])
        if raw["peak"][r] > out["peak"][k] or (raw["peak"][r] == out["peak"][k] and r < peak_from[k]):
            out["peak"][k], out["xpeak"][k], out["ypeak"][k] = raw["peak"][r], raw["xpeak"][r], raw["ypeak"][r]
            peak_from[k] = r
        if raw["vpeak"][r] > out["vpeak"][k] or (raw["vpeak"][r] == out["vpeak"][k] and r < vpeak_from[k]):
            out["vpeak"][k], out["xvpeak"][k], out["yvpeak"][k] = raw["vpeak"][r], raw["xvpeak"][r], raw["yvpeak"][r]
            vpeak_from[k] = r
        out["xmin"][k] = min(out["xmin"][k], raw["xmin"][r])
        out["xmax"][k] = max(out["xmax"][k], raw["xmax"][r])
        out["ymin"][k] = min(out["ymin"][k], raw["ymin"][r])
        out["ymax"][k] = max(out["ymax"][k], raw["ymax"][r])
        out["flag"][k] |= raw["flag"][r] | MERGED
        out["nmerged"][k] += 1
    seg = obj["segmap"]
    lut = np.concatenate([[0], newrow[root] + 1]).astype(np.int32)
    out["segmap"] = lut[seg]
    out.update(n_raw=n, absorber=absorber, root=root, survivors=survivors, mthresh_raw=mth, tables=tab, raw=raw,
               flux_abs=np.array([np.abs(t).sum() for t in flux_terms]),
               dflux_abs=np.array([np.abs(t).sum() for t in dflux_terms]))
    return out


def check_premises(res, absorbed=True, survivor_in_zone=True):
    """The premises under which the set memberships are exact whatever pow the device has - conditions on the restatement's
    own numbers, never relaxed.  absorbed / survivor_in_zone: the structure the case exists for."""
    tab, mth = res["tables"], res["mthresh_raw"]
    zone, P, val = tab["zone"], tab["P"], tab["val"]
    n = len(mth)
    m = np.broadcast_to(mth[:, None], P.shape)
    # every pair inside the zone: P clear of mthresh
    assert (np.abs(P - m)[zone] >= 1e-6 * np.maximum(P, m)[zone]).all(), "P against mthresh"
    # the best candidate clear of the second (an exact tie of identical objects is decided by the row, not by pow)
    for i in range(n):
        p = np.sort(P[i, tab["cand"][i]])
        if len(p) >= 2 and p[-1] != p[-2]:
            assert p[-1] - p[-2] >= 1e-6 * p[-1], ("best against second", i)
    # dflux of zone partners: exactly equal or clear
    df = res["raw"]["dflux"]
    a, b = np.broadcast_to(df[:, None], P.shape), np.broadcast_to(df[None, :], P.shape)
    both = zone | zone.T
    assert ((a == b) | (np.abs(a - b) >= 1e-9 * np.maximum(np.abs(a), np.abs(b))))[both].all(), "dflux of partners"
    # val clear of 1 and of 1e10
    v = val[zone]
    assert (np.abs(v - 1.0) >= 1e-6).all() and (np.abs(v - 1e10) >= 1e-6 * 1e10).all(), "val"
    # beside the four of DESIGN 7zc: the zone's own bound, clear by 1e-9 relative for every ordered pair of the field
    pr = tab["profile"]
    d2 = (res["raw"]["x_iso"][:, None] - res["raw"]["x_iso"][None, :]) ** 2 + (res["raw"]["y_iso"][:, None]
                                                                              - res["raw"]["y_iso"][None, :]) ** 2
    lim = 100.0 * (pr["a"][:, None] + pr["a"][None, :]) ** 2
    off = ~np.eye(n, dtype=bool)
    assert (np.abs(d2 - lim)[off] >= 1e-9 * lim[off]).all(), "the zone's bound"
    if absorbed:
        assert (res["root"] != np.arange(n)).any(), "nothing is absorbed"
    if survivor_in_zone:
        surv = res["root"] == np.arange(n)
        assert (zone & surv[:, None]).any(), "no survivor inside a zone"


# ---- painted fields (tests/detect_shapes.py's regime: back == 0, D == data with kernel [[1]], unit weights, noise "absolute";
# thresh 0.75 so that T = 0.75 exactly and a pixel of 1 lies 0.25 above it) ----------------------------------------------
K1 = np.array([[1.0]])
T_PAINTED = 0.75
PAINTED_KW = dict(noise="absolute", filter_type="conv", thresh=T_PAINTED, filter_kernel=K1)


def _square(d, cy, cx, half, value):
    d[cy - half:cy + half + 1, cx - half:cx + half + 1] = value


def _mesas(d, cy, cx):
    """nested mesas of 1 / 3 / 7 with half-widths 10 / 7 / 4: one object of 441 pixels"""
    for value, half in ((1, 10), (3, 7), (7, 4)):
        _square(d, cy, cx, half, value)


def motivating(H=96, W=120, cy=48, cx=60, near=True, far=True, mesas=True):
    """the nested mesas with a 2 x 2 blob of 1s (mthresh 0.25 at minarea 4) 8 px to their right and another 14 px to their
    left: at clean_param 0.5 / 1 / 2 the mesas' profile is 0.457 / 0.292 / 0.153 at the near blob and 0.349 / 0.174 / 0.059
    at the far one.  Catalogue order (by first pixel): mesas, far blob, near blob."""
    d = np.zeros((H, W))
    if mesas:
        _mesas(d, cy, cx)
    if near:
        d[cy:cy + 2, cx + 10 + 8 + 1:cx + 10 + 8 + 3] = 1
    if far:
        d[cy:cy + 2, cx - 10 - 14 - 2:cx - 10 - 14] = 1
    return d


def chain(H=96, W=120, cy=48, cx=30):
    """A the nested mesas; B a 7 x 7 square of 1 with one pixel of 10, 6 px from A; C a 2 x 2 blob 2 px from B.  At
    clean_param 1 A's profile is 0.279 at B and 0.161 at C, B's is 0.333 at C: C goes to B, B to A, all end in A."""
    d = np.zeros((H, W))
    _mesas(d, cy, cx)
    cb = cx + 10 + 6 + 1 + 3
    _square(d, cy, cb, 3, 1)
    d[cy, cb] = 10
    c0 = cb + 3 + 2 + 1
    d[cy:cy + 2, c0:c0 + 2] = 1
    return d


def tie(H=96, W=120, cy=48, cx=40):
    """two identical 7 x 7 squares of 1 with a centre of 5, 2 px apart: at clean_param 0.5 each one's profile at the other
    is 0.344 > 0.25 and their dflux are equal bit for bit: the smaller row absorbs the larger"""
    d = np.zeros((H, W))
    for c in (cx, cx + 7 + 2):
        _square(d, cy, c, 3, 1)
        d[cy, c] = 5
    return d


def crowd(H=125, W=157, cy=31, cx=104, half=24):
    """for minarea 1: nested mesas of 1 / 3 / 50 of 49 x 49 pixels (2401: the deblender's global-scratch path) inside a
    lattice of single pixels of 1 on every second row and column of rows 1 .. 63, columns 41 .. 155 - each an object of its
    own with mthresh 0.25, more than a thousand of them inside the mesas' wings - above the comb of tests/detect_shapes.py,
    whose object list and catalogue are in different orders"""
    from tests import detect_shapes as ds

    d = ds._comb()
    assert (H, W) == d.shape
    rr, cc = np.meshgrid(np.arange(1, 64, 2), np.arange(41, W, 2), indexing="ij")
    d[rr, cc] = 1
    d[cy - half - 1:cy + half + 2, cx - half - 1:cx + half + 2] = 0
    _square(d, cy, cx, half, 1)
    _square(d, cy, cx, 2 * half // 3, 3)
    _square(d, cy, cx, half // 3, 50)
    return d


def lattice_alone(H=125, W=157):
    """the right half of the lattice of crowd() without the mesas and the comb: nothing is absorbed"""
    d = np.zeros((H, W))
    rr, cc = np.meshgrid(np.arange(1, 64, 2), np.arange(101, W, 2), indexing="ij")
    d[rr, cc] = 1
    return d


def painted(data, minarea=4, clean_param=1.0):
    """(exp, obj, cleaned) of one painted field on the weighted path"""
    exp, obj, _ = oo.detect_weighted(data, np.ones_like(data), minarea=minarea, **PAINTED_KW)
    assert (exp["back"] == 0.0).all() and np.array_equal(exp["D"], data)
    return exp, obj, clean(exp, obj, exp["D"], T_PAINTED, minarea, clean_param)


# ---- the noise scenes of DESIGN 7z / 7za with faint companions in the wings of their bright sources ------------------------
# (amplitude in units of the noise, distance in pixels): tuned on the CPU until some seed of each path held the premises with
# one companion absorbed; conditions on the scene, not measurements of the detector
COMPANIONS = dict(unweighted=(8.0, 9), weighted=(6.0, 8), multiband=(4.0, 8))


def _blobs(H, W, positions, amps, sigma=1.2):
    y, x = np.mgrid[:H, :W]
    out = np.zeros((H, W))
    for (cy, cx), a in zip(positions, amps):
        out += a * np.exp(-0.5 * ((x - cx) ** 2 + (y - cy) ** 2) / sigma ** 2)
    return out


def noise_case(path, seed):
    """One 96 x 120 noise scene: (fields as the call takes them, the call's keywords, exp, obj, details, T).  unweighted: band
    2 of the multi-band scene; weighted: the scene with defects and its inverse variances; multiband: all six bands with their
    variance planes."""
    from tests import detect_multiband_oracle as mo
    from tests import detect_weighted_oracle as wo

    A, dist = COMPANIONS[path]
    if path == "unweighted":
        d = mo.scene(seed=seed)[0][:, :, 2] + _blobs(96, 120, [(16, 20 + dist), (40 + dist, 30), (70, 60 + dist)], [A] * 3)
        kw = dict(back_size=32)
        exp, obj, details = oo.detect(d, **kw)
        return d, kw, exp, obj, details, 1.5 * exp["globalrms"]
    if path == "weighted":
        data, w, _, _ = wo.scene(seed=seed)
        data = data + _blobs(96, 120, [(14, 20 + dist), (40 + dist, 30), (20, 80 + dist), (50 + dist, 104)], [A, A, 3 * A, 3 * A])
        kw = dict(weights=w, back_size=32, filter_type="conv", noise="absolute", thresh=1.5)
        exp, obj, details = oo.detect_weighted(data, w, **{k: v for k, v in kw.items() if k != "weights"})
        return data, kw, exp, obj, details, 1.5
    f = mo.scene(seed=seed)[0].copy()
    planes = mo.variance_planes()
    b = _blobs(96, 120, [(16, 20 + dist), (40 + dist, 30), (20, 84 + dist)], [1.0] * 3)
    for k in range(6):
        f[:, :, k] += A * mo.SIGMAS[k] * 0.6 * b
    kw = dict(weights=planes, noise="absolute", thresh=mo.THRESH, back_size=mo.BACK_SIZE)
    exp, obj, details = oo.detect_multiband(f, planes=planes, **{k: v for k, v in kw.items() if k != "weights"})
    return f, kw, exp, obj, details, mo.THRESH


def first_noise_case(path, seeds=range(11, 41)):
    """the case of the first seed whose premises hold (the detector's P3 / P4 and the cleaning pass's), with its cleaned
    restatement: (seed, fields, kw, exp, obj, res)"""
    for seed in seeds:
        fields, kw, exp, obj, details, T = noise_case(path, seed)
        try:
            oo.check_p3_p4(details)
            res = clean(exp, obj, exp["D"], T, 4, 1.0)
            check_premises(res)
        except AssertionError:
            continue
        return seed, fields, kw, exp, obj, res
    raise AssertionError(f"no seed of {path} holds the premises")


def loop_fields(F=119, nb=6):
    """two F-px fields (2, F, F, nb) for the iterative loop: bright blobs on noise of 0.05, each with a faint companion 10 px
    away that only the blob's wings lift over the threshold of the pass's detector"""
    rng = np.random.default_rng(31)
    fields = rng.normal(0, 0.05, (2, F, F, nb))
    for m, blobs in enumerate((((40, 45, 2.0, 6.0), (75, 50, 2.5, 8.0), (60, 75, 2.0, 5.0)), ((50, 40, 2.0, 7.0), (80, 75, 3.0, 9.0)))):
        for r, c, s, a in blobs:
            fields[m] += (_blobs(F, F, [(r, c)], [a], s) + _blobs(F, F, [(r, c + 10)], [0.3], 1.0))[:, :, None]
    return fields
