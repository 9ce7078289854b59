"""float64 numpy restatement of source detection with a per-pixel noise map and a mask: the spec
the weighted GPU detector (Context.scene_detect(weights=..., mask=...), dv_scene_detect_weighted) is tested against.

The rules of tests/detect_oracle.py with these changes.  A pixel counts iff 0 < w < inf.  Only counting pixels
enter a mesh's clipping; a mesh is good iff 2 n_counting >= its pixels; a bad mesh takes, for background and rms separately,
the mean of the good meshes at the smallest squared mesh distance (ties added in raster order), before the median filter.
v = data - back where the pixel counts, 0 elsewhere.  The significance map S stands where D stood: conv
S = (sum kn v) sqrt(w), matched S = (sum kn (v w)) / sqrt(sum (kn kn) w), -inf where the pixel does not count or the
denominator is 0.  T = thresh (noise "absolute") or thresh * globalrms ("relative").  A data value under a pixel that does
not count reaches no sum: selects, never a product with zero."""
import numpy as np

from tests.detect_oracle import (CAT_KEYS, _components, deblend_component, default_kernel, interpolate, median_filter_grid,
                                 mesh_stats)


def counting(w):
    with np.errstate(invalid="ignore"):
        return (w > 0) & (w < np.inf)


def fill_bad(grid, good):
    """the grid with every bad mesh replaced by the mean of the good meshes at the smallest di^2 + dj^2, the tied ones added
    in raster order and the sum divided by their count; NaN everywhere without a good mesh"""
    ny, nx = grid.shape
    out = grid.copy()
    gi, gj = np.nonzero(good)                                # raster order
    for i in range(ny):
        for j in range(nx):
            if good[i, j]:
                continue
            if len(gi) == 0:
                out[i, j] = np.nan
                continue
            d = (gi - i) ** 2 + (gj - j) ** 2
            s, n = 0.0, 0
            for a, b in zip(gi[d == d.min()], gj[d == d.min()]):
                s += grid[a, b]
                n += 1
            out[i, j] = s / n
    return out


def background(data, w, bs=64, fs=3):
    H, W = data.shape
    on = counting(w)
    ny, nx = -(-H // bs), -(-W // bs)
    b = np.full((ny, nx), np.nan)
    r = np.full((ny, nx), np.nan)
    good = np.zeros((ny, nx), dtype=bool)
    for i in range(ny):
        for j in range(nx):
            sl = (slice(i * bs, (i + 1) * bs), slice(j * bs, (j + 1) * bs))
            m = on[sl]
            if 2 * int(m.sum()) >= m.size:
                good[i, j] = True
                b[i, j], r[i, j] = mesh_stats(data[sl][m])
    with np.errstate(invalid="ignore"):
        fb, fr = median_filter_grid(fill_bad(b, good), fs), median_filter_grid(fill_bad(r, good), fs)
        return dict(mesh_back=fb, mesh_rms=fr, globalrms=fr.mean(), back=interpolate(fb, H, W, bs),
                    rms=interpolate(fr, H, W, bs), bad_meshes=int((~good).sum()), good=good)


def _correlate(img, taps):
    """correlation of img with the taps as given, zero outside the field; taps added in row-major order"""
    kh, kw = taps.shape
    H, W = img.shape
    p = np.pad(img, ((kh // 2, kh // 2), (kw // 2, kw // 2)))
    out = np.zeros_like(img)
    for a in range(kh):
        for b in range(kw):
            out += taps[a, b] * p[a:a + H, b:b + W]
    return out


def significance(v, w, kernel, filter_type):
    """S from v (zero where the pixel does not count) and the weights"""
    k = np.asarray(kernel, dtype=np.float64)
    kn = k / np.abs(k).sum()
    on = counting(w)
    wz = np.where(on, w, 0.0)
    if filter_type == "conv":
        S = _correlate(v, kn) * np.sqrt(wz)
    else:
        num = _correlate(np.where(on, v * wz, 0.0), kn)
        den = _correlate(wz, kn * kn)
        ok = den > 0
        S = np.full(v.shape, -np.inf)
        S[ok] = num[ok] / np.sqrt(den[ok])
    S[~on] = -np.inf
    return S


def detect(data, weights, noise="absolute", filter_type="conv", thresh=1.5, minarea=4, nthresh=64, cont=1e-5,
           filter_kernel=None, back_size=64, back_filter=3, details=None):
    """detect_oracle.detect with the weighted rules; the D map holds S; gains bad_meshes; details as there"""
    assert noise in ("absolute", "relative") and filter_type in ("conv", "matched")
    data = np.asarray(data, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    H, W = data.shape
    on = counting(w)
    bk = background(data, w, back_size, back_filter)
    labels = np.full(H * W, -1, dtype=np.int64)
    cat = {k: [] for k in CAT_KEYS}
    if not bk["good"].any():                                 # a field without a good mesh: no objects, globalrms NaN
        out = {k: np.asarray(val, dtype=np.int64 if k in ("npix", "parent") else np.float64) for k, val in cat.items()}
        out.update(back=bk["back"], rms=bk["rms"], v=np.zeros((H, W)), D=np.full((H, W), -np.inf),
                   labels=labels.reshape(H, W), globalrms=np.nan, bad_meshes=bk["bad_meshes"])
        return out
    v = np.zeros((H, W))
    v[on] = data[on] - bk["back"][on]
    S = significance(v, w, default_kernel() if filter_kernel is None else filter_kernel, filter_type)
    T = thresh if noise == "absolute" else thresh * bk["globalrms"]
    vf, Sf = v.ravel(), S.ravel()
    for pix in _components(S > T):
        if len(pix) < minarea:
            continue
        labels[pix] = pix[0]
        det = None if details is None else dict(pix=pix, T=T)
        objs, assign = deblend_component(pix, S, W, T, nthresh, minarea, cont, details=det)
        rows = []
        for o in range(len(objs)):
            p = pix[assign == o]
            sp = Sf[p]
            pk = int(np.argmax(sp))
            vv = vf[p]
            sv = vv.sum()
            r, c = p // W, p % W
            if sv > 0:
                x, y = (vv * c).sum() / sv, (vv * r).sum() / sv
            else:
                x, y = c.mean(), r.mean()
            rows.append((int(p[pk]), len(p), sp[pk], sv, x, y))
        if det is not None:
            det.update(peak_pixels=[e[0] for e in rows], assign=assign)
            details.append(det)
        for _, n, peak, sv, x, y in sorted(rows, key=lambda e: e[0]):
            for key, val in zip(CAT_KEYS, (n, peak, sv, x, y, int(pix[0]))):
                cat[key].append(val)
    out = {k: np.asarray(val, dtype=np.int64 if k in ("npix", "parent") else np.float64) for k, val in cat.items()}
    out.update(back=bk["back"], rms=bk["rms"], v=v, D=S, labels=labels.reshape(H, W), globalrms=bk["globalrms"],
               bad_meshes=bk["bad_meshes"])
    return out


def scene(seed=11, H=96, W=120):
    """the 96 x 120 test scene of DESIGN 7z: six planted sources, the right half at 3 x the noise of the left, one saturated
    column, a 7 x 10 NaN block, 24 of the 32 rows of one 32-px mesh saturated.  Returns (data, weights (inverse variance, 0
    under the defects), mask (True = bad), planted (row, column) positions)."""
    rng = np.random.default_rng(seed)
    sigma = np.where(np.arange(W) < W // 2, 1.0, 3.0)[None, :] * np.ones((H, 1))
    data = 50.0 + rng.normal(0.0, 1.0, (H, W)) * sigma
    planted = [(14, 20), (40, 30), (80, 45), (20, 80), (50, 104), (75, 100)]
    y, x = np.mgrid[:H, :W]
    for (cy, cx) in planted:
        amp = 40.0 if cx < W // 2 else 120.0
        data += amp * np.exp(-0.5 * ((x - cx) ** 2 + (y - cy) ** 2) / 2.0 ** 2)
    mask = np.zeros((H, W), dtype=bool)
    mask[:, 52] = True                                       # the bleed column
    data[:, 52] = 6.0e4
    mask[30:37, 5:15] = True                                 # a NaN block
    data[30:37, 5:15] = np.nan
    mask[64:88, 64:96] = True                                # 24 of the 32 rows of mesh (2, 2)
    data[64:88, 64:96] = 6.0e4
    weights = np.where(mask, 0.0, 1.0 / sigma ** 2)
    return data, weights, mask, np.array(planted, dtype=np.float64)
