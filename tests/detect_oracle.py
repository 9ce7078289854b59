"""float64 numpy restatement of the source detector: the spec the GPU detector
(debvader_amd/csrc/detect.hip, Context.scene_detect) is tested against.

SExtractor's published method (Bertin & Arnouts 1996) with the rules of DESIGN 7e: sigma-clipped mesh background with
exact medians, a median filter over the meshes, natural-cubic-spline interpolation, a matched filter normalised by sum|k|,
8-connected segmentation above thresh * globalrms, multi-threshold deblending with an argmax pixel assignment.  It is not
sep and is not claimed to match sep bit for bit (INTEGRATION.md lists the differences)."""
import numpy as np
import scipy.ndimage
from scipy.special import erf

EIGHT = np.ones((3, 3), dtype=bool)
DEFAULT_SIGMA = 1.27627


def default_kernel(sigma=DEFAULT_SIGMA, radius=3):
    """pixel-integrated circular Gaussian, (2 radius + 1)^2 taps (the detector divides by sum|k|)"""
    x = np.arange(-radius, radius + 1, dtype=np.float64)
    s = np.sqrt(2.0) * sigma
    g = erf((x + 0.5) / s) - erf((x - 0.5) / s)
    return np.outer(g, g)


def _median_sorted(s):
    n = len(s)
    return s[n // 2] if n % 2 else 0.5 * (s[n // 2 - 1] + s[n // 2])


def _mean_sigma(x):
    n = len(x)
    mean = x.sum() / n
    return mean, np.sqrt(np.square(x - mean).sum() / n)


def mesh_stats(vals, details=None):
    """(background, rms) of one mesh: 3-sigma clipping around the exact median, repeated until the kept set does not
    change, at most 100 rounds; every kept set is a contiguous range of the sorted values.  A dict given as details
    gains the final kept set and its mean, med and sig."""
    s = np.sort(np.asarray(vals, dtype=np.float64).ravel())
    lo, hi = 0, len(s)
    for _ in range(100):
        x = s[lo:hi]
        mean, sig = _mean_sigma(x)
        med = _median_sorted(x)
        nlo = max(lo, int(np.searchsorted(s, med - 3.0 * sig, side="left")))
        nhi = min(hi, int(np.searchsorted(s, med + 3.0 * sig, side="right")))
        if nlo == lo and nhi == hi:
            break
        lo, hi = nlo, nhi
    x = s[lo:hi]
    mean, sig = _mean_sigma(x)
    med = _median_sorted(x)
    back = 2.5 * med - 1.5 * mean if abs(mean - med) < 0.3 * sig else med
    if details is not None:
        details.update(mean=mean, med=med, sig=sig, kept=x)
    return back, sig


def median_filter_grid(g, fs):
    """fs x fs median over the mesh grid, the window clipped at the grid's edge"""
    ny, nx = g.shape
    h = fs // 2
    out = np.empty_like(g)
    for i in range(ny):
        for j in range(nx):
            out[i, j] = _median_sorted(np.sort(g[max(0, i - h):i + h + 1, max(0, j - h):j + h + 1].ravel()))
    return out


def spline_d2(y):
    """second derivatives of the natural cubic spline through y[0..n) at unit spacing, along axis 0 (Thomas algorithm)"""
    y = np.asarray(y, dtype=np.float64)
    n = y.shape[0]
    m = np.zeros_like(y)
    if n < 3:
        return m
    k = n - 2
    c = np.zeros(k)
    d = np.zeros((k,) + y.shape[1:])
    for i in range(k):
        r = 6.0 * (y[i + 2] - 2.0 * y[i + 1] + y[i])
        if i == 0:
            c[i] = 0.25
            d[i] = r * 0.25
        else:
            c[i] = 1.0 / (4.0 - c[i - 1])
            d[i] = (r - d[i - 1]) * c[i]
    m[k] = d[k - 1]
    for i in range(k - 2, -1, -1):
        m[i + 1] = d[i] - c[i] * m[i + 2]
    return m


def spline_eval(y, m, u):
    """the spline (values y, second derivatives m, along axis 0) at coordinates u; the end cubics extend outside"""
    n = y.shape[0]
    u = np.asarray(u, dtype=np.float64)
    if n == 1:
        return np.broadcast_to(y[0], u.shape + y.shape[1:]).copy()
    k = np.clip(np.floor(u), 0, n - 2).astype(np.int64)
    t = (u - k).reshape(u.shape + (1,) * (y.ndim - 1))
    a = 1.0 - t
    return a * y[k] + t * y[k + 1] + (a * a * a - a) * m[k] / 6.0 + (t * t * t - t) * m[k + 1] / 6.0


def interpolate(grid, H, W, bs):
    """pixel map from mesh values: splines along the mesh rows for every mesh column, then along the columns for every
    pixel row; mesh coordinate u = (pixel + 0.5) / bs - 0.5"""
    ur = (np.arange(H) + 0.5) / bs - 0.5
    uc = (np.arange(W) + 0.5) / bs - 0.5
    g = spline_eval(grid, spline_d2(grid), ur)          # (H, nx)
    gt = np.ascontiguousarray(g.T)                      # (nx, H)
    return spline_eval(gt, spline_d2(gt), uc).T         # (H, W)


def background(data, bs=64, fs=3):
    data = np.asarray(data, dtype=np.float64)
    H, W = data.shape
    ny, nx = -(-H // bs), -(-W // bs)
    b = np.empty((ny, nx))
    r = np.empty((ny, nx))
    for i in range(ny):
        for j in range(nx):
            b[i, j], r[i, j] = mesh_stats(data[i * bs:(i + 1) * bs, j * bs:(j + 1) * bs])
    fb, fr = median_filter_grid(b, fs), median_filter_grid(r, fs)
    return dict(mesh_back=fb, mesh_rms=fr, globalrms=fr.mean(), back=interpolate(fb, H, W, bs),
                rms=interpolate(fr, H, W, bs))


def matched_filter(v, kernel):
    """correlation of v with kernel / sum|kernel|, zero outside the field; taps added in row-major order"""
    k = np.asarray(kernel, dtype=np.float64)
    k = k / np.abs(k).sum()
    kh, kw = k.shape
    H, W = v.shape
    p = np.pad(v, ((kh // 2, kh // 2), (kw // 2, kw // 2)))
    D = np.zeros_like(v)
    for a in range(kh):
        for b in range(kw):
            D += k[a, b] * p[a:a + H, b:b + W]
    return D


def _components(mask):
    """8-connected components of mask as arrays of raster indices (ascending), ordered by their first pixel"""
    lab, n = scipy.ndimage.label(mask, structure=EIGHT)
    if n == 0:
        return []
    flat = lab.ravel()
    idx = np.nonzero(flat)[0]
    order = np.argsort(flat[idx], kind="stable")
    groups = np.split(idx[order], np.cumsum(np.bincount(flat[idx], minlength=n + 1)[1:])[:-1])
    return sorted(groups, key=lambda g: g[0])


def deblend_component(pix, D, W, T, nthresh, minarea, cont, details=None):
    """multi-threshold deblending of one component (pixels pix, ascending raster indices).  Returns the final objects as
    (core mask over pix, threshold of the core's level) and the object every pixel of pix is assigned to.  A dict given as
    details is filled with what the rules went through (tests/detect_shapes.py checks its premises on it): values (D over
    pix), levels (every t_k computed), nobj (the length of the object list after each of them), split_levels (the k at
    which an object was replaced), core_first (the first pixel of every final object's core, in the order of the object
    list), score (objects x pixels, None for one object) and free (the pixels assigned by score); no returned value
    depends on it."""
    Dp = D.ravel()[pix]
    rows, cols = pix // W, pix % W
    r0, c0 = rows.min(), cols.min()
    sub = np.zeros((rows.max() - r0 + 1, cols.max() - c0 + 1), dtype=bool)
    P = Dp.max()
    cflux = Dp.sum()
    objs = [(np.ones(len(pix), dtype=bool), T)]
    if details is not None:
        details.update(values=Dp, levels=[], nobj=[], split_levels=[], score=None, free=np.zeros(len(pix), dtype=bool))
    for k in range(1, nthresh):
        t = T * (P / T) ** (k / nthresh)
        if details is not None:
            details["levels"].append(t)
            details["nobj"].append(len(objs))
        above = Dp > t
        if above.sum() < minarea:            # no node at this level or above
            break
        sub[:] = False
        sub[rows[above] - r0, cols[above] - c0] = True
        lab, n = scipy.ndimage.label(sub, structure=EIGHT)
        pl = lab[rows - r0, cols - c0]
        nodes = []
        for li in range(1, n + 1):
            m = pl == li
            if m.sum() >= minarea:
                nodes.append((int(np.argmax(m)), m))     # (first pixel, mask)
        nodes.sort(key=lambda e: e[0])
        new = []
        for om, ot in objs:
            sig = [m for first, m in nodes if om[first] and Dp[m].sum() > cont * cflux]
            if len(sig) >= 2:
                new += [(m, t) for m in sig]
            else:
                new.append((om, ot))
        if details is not None:
            details["nobj"][-1] = len(new)
            if len(new) != len(objs):
                details["split_levels"].append(k)
        objs = new
    assign = np.full(len(pix), -1, dtype=np.int64)
    if details is not None:
        details["core_first"] = [int(pix[np.argmax(m)]) for m, _ in objs]
    if len(objs) == 1:
        assign[:] = 0
        return objs, assign
    score = np.full((len(objs), len(pix)), -np.inf)
    for o, (m, t) in enumerate(objs):
        assign[m] = o
        w = Dp[m] - t
        sw = w.sum()
        mx, my = (w * cols[m]).sum() / sw, (w * rows[m]).sum() / sw
        dx, dy = cols[m] - mx, rows[m] - my
        sxx = (w * dx * dx).sum() / sw + 1.0 / 12.0
        syy = (w * dy * dy).sum() / sw + 1.0 / 12.0
        sxy = (w * dx * dy).sum() / sw
        det = sxx * syy - sxy * sxy
        A = Dp[m].max()
        ex, ey = cols - mx, rows - my
        q = (syy * ex * ex - 2.0 * sxy * ex * ey + sxx * ey * ey) / det
        score[o] = A * np.exp(-0.5 * q)
    free = assign < 0
    if details is not None:
        details.update(score=score, free=free)
    assign[free] = np.argmax(score[:, free], axis=0)     # the first maximum: ties go to the earlier object
    return objs, assign


CAT_KEYS = ("npix", "peak", "flux", "x", "y", "parent")


def detect(data, thresh=1.5, minarea=4, nthresh=64, cont=1e-5, filter_kernel=None, back_size=64, back_filter=3,
           details=None):
    """one field (H, W) -> dict with the maps back, rms, v, D, labels (raster index of the component's first pixel for
    the pixels of every component of >= minarea pixels, -1 elsewhere), globalrms and the catalog npix, peak, flux, x
    (column), y (row), parent (the component's label); objects ordered by component, then by peak pixel.  A list given
    as details gains one dict per kept component: deblend_component's, plus pix, T, assign and peak_pixels (every object's
    peak pixel, in the order of the object list; the catalogue's order is the sorted one)."""
    data = np.asarray(data, dtype=np.float64)
    H, W = data.shape
    bk = background(data, back_size, back_filter)
    v = data - bk["back"]
    D = matched_filter(v, default_kernel() if filter_kernel is None else filter_kernel)
    T = thresh * bk["globalrms"]
    labels = np.full(H * W, -1, dtype=np.int64)
    cat = {k: [] for k in CAT_KEYS}
    vf, Df = v.ravel(), D.ravel()
    for pix in _components(D > T):
        if len(pix) < minarea:
            continue
        labels[pix] = pix[0]
        det = None if details is None else dict(pix=pix, T=T)
        objs, assign = deblend_component(pix, D, W, T, nthresh, minarea, cont, details=det)
        rows = []
        for o in range(len(objs)):
            p = pix[assign == o]
            dp = Df[p]
            pk = int(np.argmax(dp))
            vv = vf[p]
            sv = vv.sum()
            r, c = p // W, p % W
            if sv > 0:
                x, y = (vv * c).sum() / sv, (vv * r).sum() / sv
            else:
                x, y = c.mean(), r.mean()
            rows.append((int(p[pk]), len(p), dp[pk], sv, x, y))
        if det is not None:
            det.update(peak_pixels=[e[0] for e in rows], assign=assign)
            details.append(det)
        for _, n, peak, sv, x, y in sorted(rows, key=lambda e: e[0]):
            for key, val in zip(CAT_KEYS, (n, peak, sv, x, y, int(pix[0]))):
                cat[key].append(val)
    out = {k: np.asarray(val, dtype=np.int64 if k in ("npix", "parent") else np.float64) for k, val in cat.items()}
    out.update(back=bk["back"], rms=bk["rms"], v=v, D=D, labels=labels.reshape(H, W), globalrms=bk["globalrms"])
    return out


def detect_objects(field_image, **kw):
    """the reference's detect_objects (detect/detection.py) with this detector in place of sep"""
    F = field_image.shape[1]
    c = detect(np.asarray(field_image, dtype=np.float64)[0, :, :, 2], **kw)
    return np.array([(np.round(-int(F / 2) + y), np.round(-int(F / 2) + x)) for x, y in zip(c["x"], c["y"])])
