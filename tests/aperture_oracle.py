"""numpy float64 restatement of the aperture photometry: circular apertures, the Kron radius, the flux
in the automatic ellipse and the flux radii.  Written from the specification, not from the kernel; it is the reference of
tests/test_aperture_host.py and tests/test_gpu_aperture.py.  Every expression is written in the order the specification
gives it, numpy rounds every operation on its own, and the sums run over the pixels of positive weight in raster order
(np.cumsum adds one element after the other).  The weight w = n / s^2 of a pixel is carried as its count n: a sum of w x is
the sum of n x over s^2, and the sum of the weights adds whole numbers, which is exact in any order.  Beside the outputs a row
reports its tie margins: how close any inside / outside decision and any bisection decision came to going the other way."""
import numpy as np

OK, INELIGIBLE, NO_KRON = 0, 4, 7
FLAG_AUTO, FLAG_LIMIT, FLAG_KRON_MIN = 1 << 8, 1 << 9, 1 << 10

DEFAULTS = dict(radii=(3.0, 5.0, 8.0), fractions=(0.2, 0.5, 0.8), subsample=5, kron_factor=2.5, kron_min=3.5, kron_limit=6.0,
                bisect_iters=32)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def rsum(v):
    """the sum of v in raster order"""
    v = np.asarray(v, dtype=np.float64).ravel()
    return np.float64(np.cumsum(v)[-1]) if v.size else np.float64(0.0)


def offsets(s):
    return (np.arange(s, dtype=np.float64) + 0.5) / np.float64(s) - 0.5


def quad(form, x, y):
    a, b, c = form
    return (a * x) * x + (b * x) * y + (c * y) * y


def counts(cs, r0, c0, form, rho, s, shortcut=False):
    """(count (cs, cs) int: how many of the s x s sub-pixel centres of every pixel lie in q <= rho rho, margin: the smallest
    |q - rho rho| / (rho rho) over the sub-pixels tested).  shortcut: pixels whose centre decides are not tested."""
    a, b, c = form
    dr = (np.arange(cs, dtype=np.float64) - r0)[:, None]
    dc = (np.arange(cs, dtype=np.float64) - c0)[None, :]
    o = offsets(s)
    rho2 = rho * rho
    with np.errstate(all="ignore"):
        if shortcut:
            qc = np.sqrt(quad(form, dr, dc))
            m = 0.7072 * np.sqrt(a + c)
            inside, outside = qc + m <= rho, qc - m >= rho
            todo = ~(inside | outside)
        else:
            inside = np.zeros((cs, cs), bool)
            todo = np.ones((cs, cs), bool)
        cnt = np.where(inside, s * s, 0).astype(np.int64)
        rr, cc = np.nonzero(todo)
        margin = np.inf
        if rr.size:
            x = dr[rr, 0][:, None, None] + o[None, :, None]
            y = dc[0, cc][:, None, None] + o[None, None, :]
            q = quad(form, x, y)
            cnt[rr, cc] = (q <= rho2).sum(axis=(1, 2))
            d = np.abs(q - rho2) / rho2
            d = d[np.isfinite(d)]
            margin = float(d.min()) if d.size else np.inf
    return cnt, margin


def _leaves(r0, c0, hr, hc, cs):
    edge = np.float64(cs) - 0.5
    with np.errstate(all="ignore"):
        return bool(r0 - hr < -0.5 or r0 + hr > edge or c0 - hc < -0.5 or c0 + hc > edge)


def _region_sums(P, S, cnt, s):
    """flux (nb,), var (nb,) or None, area, abs (nb,): the sums of one region over the pixels of positive weight"""
    sel = cnt > 0
    nb = P.shape[2]
    ws, s2 = cnt[sel].astype(np.float64), np.float64(s * s)
    flux = np.array([rsum(ws * P[:, :, b][sel]) for b in range(nb)]) / s2
    ab = np.array([rsum(ws * np.abs(P[:, :, b][sel])) for b in range(nb)]) / s2
    var = None if S is None else np.array([rsum(ws * (S[:, :, b][sel] * S[:, :, b][sel])) for b in range(nb)]) / s2
    area = rsum(ws) / s2                                   # whole numbers add exactly: the area has no summation order
    return flux, var, area, ab


def aperture_row(P, S, shape, status, band=2, par=None, shortcut=False):
    """One galaxy: P (cs, cs, nb) its mean stamp, S its stddev stamp or None, shape = (r0, c0, Mrr, Mrc, Mcc), status.  Returns
    a dict of the outputs (ap_flux, ap_var - the sum under the root of ap_flux_err -, ap_flux_err, ap_area, flux_auto,
    auto_var, flux_auto_err, kron, flux_rho, flags, status), of the absolute sums the comparison bounds scale with (ap_abs,
    auto_abs, kron_abs = (sum sqrt(q) |I|, sum |I|) beside kron_sums = (sum sqrt(q) I, sum I)), of the bisection's decisions (decisions[j]: a list of bools, True where
    hi moved) and of the tie margins (margin_sub, margin_bis)."""
    par = params() if par is None else par
    P = np.asarray(P).astype(np.float64)
    S = None if S is None else np.asarray(S).astype(np.float64)
    cs, nb = P.shape[0], P.shape[2]
    R = [np.float64(v) for v in par["radii"]]
    fr = [np.float64(v) for v in par["fractions"]]
    K, J, s = len(R), len(fr), int(par["subsample"])
    nan = np.float64(np.nan)
    out = dict(ap_flux=np.full((K, nb), nan), ap_var=np.full((K, nb), nan), ap_flux_err=np.full((K, nb), nan),
               ap_area=np.full(K, nan), ap_abs=np.full((K, nb), nan), flux_auto=np.full(nb, nan), auto_var=np.full(nb, nan),
               flux_auto_err=np.full(nb, nan), auto_abs=np.full(nb, nan), kron=np.full(3, nan), kron_sums=(nan, nan), kron_abs=(nan, nan),
               flux_rho=np.full(J, nan), flags=0, status=INELIGIBLE, decisions=[[] for _ in range(J)], margin_sub=np.inf,
               margin_bis=np.inf)
    r0, c0, Mrr, Mrc, Mcc = (np.float64(v) for v in shape)
    with np.errstate(all="ignore"):
        det = Mrr * Mcc - Mrc * Mrc
        if status not in (0, 2) or not np.all(np.isfinite([r0, c0, Mrr, Mrc, Mcc])) or not (np.isfinite(det) and det > 1e-6):
            return out
        flags = 0
        margin = np.inf
        # 1. the circles
        circle = (np.float64(1.0), np.float64(0.0), np.float64(1.0))
        for k in range(K):
            if _leaves(r0, c0, R[k], R[k], cs):
                flags |= 1 << k
            cnt, mg = counts(cs, r0, c0, circle, R[k], s, shortcut)
            margin = min(margin, mg)
            out["ap_flux"][k], var, out["ap_area"][k], out["ap_abs"][k] = _region_sums(P, S, cnt, s)
            if var is not None:
                out["ap_var"][k], out["ap_flux_err"][k] = var, np.sqrt(var)
        # 2. the Kron radius
        form = (Mcc / det, (-2.0 * Mrc) / det, Mrr / det)
        sr, sc = np.sqrt(Mrr), np.sqrt(Mcc)
        lim = np.float64(par["kron_limit"])
        if _leaves(r0, c0, lim * sr, lim * sc, cs):
            flags |= FLAG_LIMIT
        I = P[:, :, band]
        dr = (np.arange(cs, dtype=np.float64) - r0)[:, None]
        dc = (np.arange(cs, dtype=np.float64) - c0)[None, :]
        q = quad(form, dr, dc)
        lim2 = lim * lim
        sel = q <= lim2
        d = np.abs(q - lim2) / lim2
        margin = min(margin, float(d[np.isfinite(d)].min()))
        A, B = rsum(np.sqrt(q[sel]) * I[sel]), rsum(I[sel])
        r1 = A / B
        out["kron_sums"] = (A, B)
        out["flags"] = flags
        out["margin_sub"] = margin
        if not (np.isfinite(B) and B > 0.0) or not np.isfinite(r1):
            out["status"] = NO_KRON
            return out
        out["kron_abs"] = (rsum(np.sqrt(q[sel]) * np.abs(I[sel])), rsum(np.abs(I[sel])))
        rho_auto = np.float64(par["kron_factor"]) * r1
        if rho_auto < np.float64(par["kron_min"]):
            rho_auto = np.float64(par["kron_min"])
            flags |= FLAG_KRON_MIN
        if _leaves(r0, c0, rho_auto * sr, rho_auto * sc, cs):
            flags |= FLAG_AUTO
        # 3. the automatic aperture
        cnt, mg = counts(cs, r0, c0, form, rho_auto, s, shortcut)
        margin = min(margin, mg)
        out["flux_auto"], var, area, out["auto_abs"] = _region_sums(P, S, cnt, s)
        if var is not None:
            out["auto_var"], out["flux_auto_err"] = var, np.sqrt(var)
        out["kron"] = np.array([r1, rho_auto, area])
        # 4. the flux radii
        fauto = out["flux_auto"][band]
        mbis = np.inf
        for j in range(J):
            t = fr[j] * fauto
            lo, hi = np.float64(0.0), rho_auto
            for _ in range(int(par["bisect_iters"])):
                mid = 0.5 * (lo + hi)
                cnt, mg = counts(cs, r0, c0, form, mid, s, shortcut)
                margin = min(margin, mg)
                sel = cnt > 0
                F = rsum(cnt[sel].astype(np.float64) * I[sel]) / np.float64(s * s)
                gap = abs(F - t) / abs(fauto)
                if np.isfinite(gap):
                    mbis = min(mbis, float(gap))
                up = bool(F >= t)
                out["decisions"][j].append(up)
                if up:
                    hi = mid
                else:
                    lo = mid
            out["flux_rho"][j] = hi
        out.update(flags=flags, status=OK, margin_sub=margin, margin_bis=mbis)
    return out


def replay(rho_auto, decisions):
    """the upper end of the bisection from [0, rho_auto] under the given decisions: exact halving"""
    lo, hi = np.float64(0.0), np.float64(rho_auto)
    for up in decisions:
        mid = 0.5 * (lo + hi)
        if up:
            hi = mid
        else:
            lo = mid
    return hi


def aperture(mean, stddev, shape, status, band=2, par=None, shortcut=False):
    """mean / stddev (N, cs, cs, nb), shape (N, 5), status (N,) -> the list of the rows' dicts"""
    return [aperture_row(mean[i], None if stddev is None else stddev[i], shape[i], int(status[i]), band, par, shortcut)
            for i in range(len(mean))]


def gaussian_truth(fractions, kron_min=3.5):
    """What a noise-free elliptical Gaussian measured in the ellipse of its own moments gives in the continuum: the Kron
    radius sqrt(pi / 2), flux_auto / flux = 1 - exp(-kron_min^2 / 2) (kron_min decides: 2.5 sqrt(pi / 2) < 3.5) and the flux
    radii sqrt(-2 ln(1 - f (1 - exp(-kron_min^2 / 2)))) in units of the ellipse."""
    enc = 1.0 - np.exp(-0.5 * kron_min * kron_min)
    f = np.asarray(fractions, dtype=np.float64)
    return np.sqrt(np.pi / 2.0), enc, np.sqrt(-2.0 * np.log(1.0 - f * enc))
