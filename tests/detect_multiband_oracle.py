"""float64 numpy restatement of multi-band source detection: the spec the GPU detector on the
inverse-variance combination of bands (Context.scene_detect_multiband, dv_scene_detect_multiband) is tested against.

Per selected band j the background of tests/detect_oracle.py (no planes) or of tests/detect_weighted_oracle.py (with the
plane P_j) gives back_j, rms_j, the band's globalrms g_j and v_j = data_j - back_j.  The band's weight is w_j = 1 / (rms_j
rms_j), P_j / (rms_j rms_j) (noise "relative") or P_j ("absolute"); band j counts at a pixel iff 0 < w_j < inf, with planes
also 0 < P_j < inf, and the band has a good mesh in the field.  Over the counting bands, j ascending and from +0.0:
num = sum (c_j w_j) v_j, Wt = sum (c_j c_j) w_j; V = 0 (no counting band: the pixel does not count), v_j / c_j (one) or
num / Wt (more).  Everything behind is detect_weighted_oracle's with (V, Wt) in the place of (v, w), absolute noise and
T = thresh.  Every product and sum is rounded on its own; a value under a band that does not count reaches no sum."""
import numpy as np

from tests import detect_oracle as do
from tests import detect_weighted_oracle as wo

NOISES = (None, "absolute", "relative")


def check_args(nb, bands, band_weights, planes_shape, noise, filter_type, thresh):
    """the refusals of the spec, as ValueError; returns (bands, c)"""
    bands = list(range(nb)) if bands is None else [int(b) for b in bands]
    if not 1 <= len(bands) <= nb:
        raise ValueError(f"1 <= k <= {nb} bands, got {len(bands)}")
    if any(b < 0 or b >= nb for b in bands) or len(set(bands)) != len(bands):
        raise ValueError(f"bands must be distinct and within 0 .. {nb - 1}, got {bands}")
    c = np.ones(len(bands)) if band_weights is None else np.asarray(band_weights, dtype=np.float64)
    if c.shape != (len(bands),) or not (np.isfinite(c) & (c > 0)).all():
        raise ValueError(f"band_weights must be {len(bands)} finite values > 0, got {band_weights}")
    if noise not in NOISES or filter_type not in ("conv", "matched"):
        raise ValueError(f"unknown noise {noise!r} or filter {filter_type!r}")
    if (planes_shape is None) != (noise is None):
        raise ValueError("noise goes with the planes")
    if not thresh > 0:
        raise ValueError(f"thresh must be > 0, got {thresh}")
    return bands, c


def combine(fields, bands=None, band_weights=None, planes=None, noise=None, back_size=64, back_filter=3):
    """steps 1 - 3 and 5 of the spec for one field (H, W, nb): dict with back, rms (H, W, k), V, Wt (H, W), counts (H, W, k),
    band_globalrms (k,), bad_meshes (k,), good (k,), globalrms"""
    fields = np.asarray(fields, dtype=np.float64)
    H, W, nb = fields.shape
    bands, c = check_args(nb, bands, band_weights, None if planes is None else np.shape(planes), noise, "conv", 1.0)
    k = len(bands)
    if planes is not None:
        planes = np.asarray(planes, dtype=np.float64)
        assert planes.shape == (H, W, k), planes.shape
    back, rms = np.empty((H, W, k)), np.empty((H, W, k))
    on_all = np.zeros((H, W, k), dtype=bool)
    g, bad, good = np.empty(k), np.zeros(k, dtype=np.int64), np.ones(k, dtype=bool)
    num, Wt, v1, c1 = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W)), np.ones((H, W))
    n = np.zeros((H, W), dtype=np.int64)
    for j, b in enumerate(bands):
        data = fields[:, :, b]
        if planes is None:
            bk = do.background(data, back_size, back_filter)
            P = None
        else:
            P = planes[:, :, j]
            bk = wo.background(data, P, back_size, back_filter)
            bad[j], good[j] = bk["bad_meshes"], bk["good"].any()
        back[:, :, j], rms[:, :, j], g[j] = bk["back"], bk["rms"], bk["globalrms"]
        with np.errstate(all="ignore"):
            if planes is None:
                w = 1.0 / (bk["rms"] * bk["rms"])
            elif noise == "relative":
                w = P / (bk["rms"] * bk["rms"])
            else:
                w = P.copy()
        on = wo.counting(w) & bool(good[j])
        if planes is not None:
            on &= wo.counting(P)
        on_all[:, :, j] = on
        ws = np.where(on, w, 1.0)                               # (selects: nothing under a band that does not count)
        v = np.zeros((H, W))
        v[on] = data[on] - bk["back"][on]
        num = np.where(on, num + (c[j] * ws) * v, num)
        Wt = np.where(on, Wt + (c[j] * c[j]) * ws, Wt)
        v1 = np.where(on, v, v1)
        c1 = np.where(on, c[j], c1)
        n += on
    V = np.zeros((H, W))
    V[n == 1] = (v1 / c1)[n == 1]
    V[n >= 2] = num[n >= 2] / Wt[n >= 2]
    Wt = np.where(n == 0, 0.0, Wt)
    acc = 0.0
    for j in range(k):
        if good[j]:
            with np.errstate(divide="ignore"):
                acc = acc + (c[j] * c[j]) / (g[j] * g[j])
    globalrms = 1.0 / np.sqrt(acc) if good.any() else np.nan
    return dict(back=back, rms=rms, V=V, Wt=Wt, counts=on_all, band_globalrms=g, bad_meshes=bad, good=good,
                globalrms=globalrms)


def detect(fields, bands=None, band_weights=None, planes=None, noise=None, filter_type="conv", thresh=1.5, minarea=4,
           nthresh=64, cont=1e-5, filter_kernel=None, back_size=64, back_filter=3):
    """one field (H, W, nb) -> combine()'s dict plus D (the significance S), labels and the catalogue of
    detect_weighted_oracle.detect, computed from (V, Wt) with absolute noise and T = thresh"""
    fields = np.asarray(fields, dtype=np.float64)
    H, W, nb = fields.shape
    check_args(nb, bands, band_weights, None if planes is None else np.shape(planes), noise, filter_type, thresh)
    out = combine(fields, bands, band_weights, planes, noise, back_size, back_filter)
    labels = np.full(H * W, -1, dtype=np.int64)
    cat = {key: [] for key in do.CAT_KEYS}
    V, Wt = out["V"], out["Wt"]
    if not out["good"].any():                                # a field without a band with a good mesh
        S = np.full((H, W), -np.inf)
    else:
        S = wo.significance(V, Wt, do.default_kernel() if filter_kernel is None else filter_kernel, filter_type)
        T = thresh
        vf, Sf = V.ravel(), S.ravel()
        for pix in do._components(S > T):
            if len(pix) < minarea:
                continue
            labels[pix] = pix[0]
            objs, assign = do.deblend_component(pix, S, W, T, nthresh, minarea, cont)
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
            for _, n, peak, sv, x, y in sorted(rows, key=lambda e: e[0]):
                for key, val in zip(do.CAT_KEYS, (n, peak, sv, x, y, int(pix[0]))):
                    cat[key].append(val)
    out.update({key: np.asarray(val, dtype=np.int64 if key in ("npix", "parent") else np.float64) for key, val in cat.items()})
    out.update(D=S, labels=labels.reshape(H, W))
    return out


# ---- the test scene ------------------------------------------------------------------------------------------------
BACKGROUNDS = (50.0, 20.0, 80.0, 10.0, 5.0, 200.0)
SIGMAS = (1.0, 1.5, 1.0, 1.25, 0.8, 2.0)
THRESH = 2.5
BACK_SIZE = 32
# The two faint amplitudes were tuned on the CPU until the conditions of tests/test_detect_multiband_host.py held on this
# oracle (they are conditions on the scene, not measurements of the detector): "faint" so that the six-band combination has
# peak S >= THRESH + 0.5 while no single band reaches THRESH - 0.4 within 6 px of it, "red" so that the flat combination
# stays under THRESH - 0.4.  With seed 11: FAINT 2.1 gave 2.94 (too low), 2.3 gives 3.25 against 1.90 in the best single band,
# 2.4 gives 3.41 against 1.99; RED 1.6 gives 1.43 flat and 2.21 with RED_WEIGHTS.
FAINT = 2.3
RED = 1.6
RED_SHAPE = (0.0, 0.0, 0.0, 0.3, 1.0, 3.0)
RED_WEIGHTS = (0.05, 0.05, 0.05, 0.3, 1.0, 3.0)
SOURCES = {                       # name: ((row, column), amplitude per band)
    "all": ((16, 20), (12.0,) * 6),
    "r_only": ((40, 30), (0.0, 0.0, 12.0, 0.0, 0.0, 0.0)),
    "not_r": ((20, 84), (12.0, 0.0, 0.0, 0.0, 12.0, 0.0)),
    "faint": ((70, 60), (FAINT,) * 6),
    "red": ((76, 100), tuple(RED * s for s in RED_SHAPE)),
}


def scene(seed=11, H=96, W=120):
    """the 96 x 120 x 6 test scene of DESIGN 7za: flat backgrounds and white noise per band, five Gaussian sources of
    sigma 2 px.  Returns (fields (H, W, 6), {name: (row, column)})."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:H, :W]
    fields = np.empty((H, W, 6))
    for b in range(6):
        fields[:, :, b] = BACKGROUNDS[b] + rng.normal(0.0, SIGMAS[b], (H, W))
    for (cy, cx), amps in SOURCES.values():
        g = np.exp(-0.5 * ((x - cx) ** 2 + (y - cy) ** 2) / 2.0 ** 2)
        for b in range(6):
            fields[:, :, b] += amps[b] * g
    return fields, {name: pos for name, (pos, _) in SOURCES.items()}


def variance_planes(H=96, W=120):
    """the inverse-variance planes of the scene's noise, (H, W, 6)"""
    return np.broadcast_to(1.0 / np.square(np.asarray(SIGMAS)), (H, W, 6)).copy()


def near(pos, H=96, W=120, radius=6.0):
    """the pixels within radius of (row, column)"""
    y, x = np.mgrid[:H, :W]
    return np.hypot(y - pos[0], x - pos[1]) <= radius
