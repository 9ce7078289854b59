"""numpy restatement of the detector's object columns and segmentation map.  numpy and scipy only.

Everything here is built from what the three detector restatements (tests/detect_oracle.py, detect_weighted_oracle.py,
detect_multiband_oracle.py) already give: their maps and, per kept component, the `details` of the deblender (pix, the
component's pixels in raster order; assign, the entry of the object list every pixel went to; peak_pixels, every entry's
peak pixel).  The sums are written in the form of the definitions, with numpy's own summation order."""
import numpy as np

from tests import detect_multiband_oracle as mo
from tests import detect_oracle as do
from tests import detect_weighted_oracle as wo

INT_KEYS = ("xmin", "xmax", "ymin", "ymax", "xpeak", "ypeak", "xvpeak", "yvpeak", "flag")
DOUBLE_KEYS = ("vpeak", "dflux", "x_iso", "y_iso", "x2", "y2", "xy")
BLENDED, BORDER, SINGULAR, MASKED = 1, 2, 4, 8


def counting(w):
    with np.errstate(invalid="ignore"):
        return (w > 0) & (w < np.inf)


def objects(details, D, v, wt=None):
    """the columns (one row per object, in catalogue order: by component, then by peak pixel), npix and the segmap of one
    field from the deblender's details, the thresholded map D, the map v that flux sums and, for flag bit 8, the weight
    plane wt whose counting pixels the weighted and the multi-band call ask about (None: the unweighted call)"""
    H, W = D.shape
    Df, vf = D.ravel(), v.ravel()
    bad = None if wt is None else ~counting(np.asarray(wt, dtype=np.float64))
    segmap = np.zeros(H * W, dtype=np.int32)
    rows = {k: [] for k in INT_KEYS + DOUBLE_KEYS + ("npix",)}
    base = 0
    for det in details:
        pix, assign, peaks = det["pix"], det["assign"], det["peak_pixels"]
        nobj = len(peaks)
        order = np.argsort(peaks)                           # catalogue position -> entry of the object list
        rank = np.empty(nobj, dtype=np.int64)
        rank[order] = np.arange(nobj)
        segmap[pix] = base + rank[assign] + 1
        base += nobj
        for o in order:
            p = pix[assign == o]
            r, c = p // W, p % W
            Dp, vp = Df[p], vf[p]
            sD = Dp.sum()
            x_iso, y_iso = (Dp * c).sum() / sD, (Dp * r).sum() / sD
            dx, dy = c - x_iso, r - y_iso
            x2, y2, xy = ((Dp * dx) * dx).sum() / sD, ((Dp * dy) * dy).sum() / sD, ((Dp * dx) * dy).sum() / sD
            flag = BLENDED if nobj > 1 else 0
            if c.min() == 0 or r.min() == 0 or c.max() == W - 1 or r.max() == H - 1:
                flag |= BORDER
            if x2 * y2 - xy * xy < 1.0 / 144.0:
                x2, y2 = x2 + 1.0 / 12.0, y2 + 1.0 / 12.0
                flag |= SINGULAR
            if bad is not None:
                hit = False
                for dr in (-1, 0, 1):
                    for dc in (-1, 0, 1):
                        if dr == 0 and dc == 0:
                            continue
                        rr, cc = r + dr, c + dc
                        inside = (rr >= 0) & (rr < H) & (cc >= 0) & (cc < W)
                        hit = hit or bool(bad[rr[inside], cc[inside]].any())
                if hit:
                    flag |= MASKED
            pk, vk = int(p[np.argmax(Dp)]), int(p[np.argmax(vp)])       # the first maximum: the smallest raster index
            assert pk == peaks[o]
            for key, val in zip(INT_KEYS + DOUBLE_KEYS + ("npix",),
                                (c.min(), c.max(), r.min(), r.max(), pk % W, pk // W, vk % W, vk // W, flag,
                                 vp.max(), sD, x_iso, y_iso, x2, y2, xy, len(p))):
                rows[key].append(val)
    out = {k: np.asarray(val, dtype=np.float64 if k in DOUBLE_KEYS else np.int32) for k, val in rows.items()}
    out["segmap"] = segmap.reshape(H, W)
    return out


def derived(x2, y2, xy):
    """a, b, theta and SExtractor's cxx, cyy, cxy from the moments"""
    x2, y2, xy = (np.asarray(e, dtype=np.float64) for e in (x2, y2, xy))
    p, d = x2 + y2, x2 - y2
    t = np.sqrt(d * d / 4.0 + xy * xy)
    det = x2 * y2 - xy * xy
    theta = np.where((xy == 0) & (d == 0), 0.0, 0.5 * np.arctan2(2.0 * xy, d))
    return dict(a=np.sqrt(p / 2.0 + t), b=np.sqrt(np.maximum(p / 2.0 - t, 0.0)), theta=theta, cxx=y2 / det, cyy=x2 / det,
                cxy=-2.0 * xy / det)


def details_of(D, T, minarea=4, nthresh=64, cont=1e-5):
    """the deblender's details of every kept component of D > T, as detect_oracle.detect collects them (for the multi-band
    restatement, whose detect() keeps none)"""
    H, W = D.shape
    Df = D.ravel()
    out = []
    for pix in do._components(D > T):
        if len(pix) < minarea:
            continue
        det = dict(pix=pix, T=T)
        objs, assign = do.deblend_component(pix, D, W, T, nthresh, minarea, cont, details=det)
        det.update(assign=assign, peak_pixels=[int(pix[assign == o][np.argmax(Df[pix[assign == o]])])
                                               for o in range(len(objs))])
        out.append(det)
    return out


def detect(data, **kw):
    """detect_oracle.detect plus the objects: (result, objects)"""
    details = []
    exp = do.detect(data, details=details, **kw)
    return exp, objects(details, exp["D"], exp["v"]), details


def detect_weighted(data, weights, **kw):
    details = []
    exp = wo.detect(data, weights, details=details, **kw)
    return exp, objects(details, exp["D"], exp["v"], wt=weights), details


def detect_multiband(fields, **kw):
    exp = mo.detect(fields, **kw)
    details = details_of(exp["D"], kw.get("thresh", 1.5), kw.get("minarea", 4), kw.get("nthresh", 64), kw.get("cont", 1e-5))
    obj = objects(details, exp["D"], exp["V"], wt=exp["Wt"])
    assert np.array_equal(obj["npix"], exp["npix"])          # the details are those of mo.detect's own loop
    return exp, obj, details


def check_p3_p4(details):
    """the premises P3 and P4 of tests/detect_shapes.check_premises, which make every set membership exact: no pixel value
    within 1e-6 P of a level its component reaches, every pixel assigned by score 1e-6 (relative) clear of the second best"""
    for c in details:
        vals = np.unique(c["values"])
        gap = np.abs(vals[:, None] - np.asarray(c["levels"])[None, :]).min() if len(c["levels"]) else np.inf
        assert gap >= 1e-6 * vals.max(), ("P3", int(c["pix"][0]), gap)
        if c["score"] is not None and c["free"].any():
            s = np.sort(c["score"][:, c["free"]], axis=0)
            assert (s[-1] > 0.0).all() and (s[-1] - s[-2] >= 1e-6 * s[-1]).all(), ("P4", int(c["pix"][0]))
