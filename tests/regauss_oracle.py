"""numpy float64 restatement of the PSF correction: re-Gaussianization after Hirata & Seljak (2003),
ending in a plain moment subtraction.  Written from the specification, not from the kernel; it is the reference of
tests/test_regauss_host.py and tests/test_gpu_regauss.py.  The iteration is tests/measure_oracle.py's, restated here with a
start state (adaptive_moments_from; test_regauss_host.py holds the two to the same bits from the default start)."""
import numpy as np

from tests import measure_oracle as mo

CONVERGED, ITER_LIMIT, FAILED, INELIGIBLE, NO_PSF, UNRESOLVED = 0, 2, 3, 4, 5, 6


def adaptive_moments_from(I, start, tol=1e-10, max_iter=200):
    """measure_oracle.adaptive_moments from the state start = (r0, c0, Mrr, Mrc, Mcc) instead of the stamp centre and sigma0"""
    I = np.asarray(I, dtype=np.float64)
    cs = I.shape[0]
    assert I.shape == (cs, cs)
    r = np.arange(cs, dtype=np.float64)[:, None]
    c = np.arange(cs, dtype=np.float64)[None, :]
    ctr = (cs - 1) / 2.0
    r0, c0, Mrr, Mrc, Mcc = (float(v) for v in start)
    it, status = 0, ITER_LIMIT
    with np.errstate(all="ignore"):
        for k in range(1, int(max_iter) + 1):
            it = k
            det = Mrr * Mcc - Mrc * Mrc
            if not np.isfinite(det) or not det > 1e-6:
                status = FAILED
                break
            dr, dc = r - r0, c - c0
            w = np.exp(-0.5 * (Mcc * dr * dr - 2.0 * Mrc * dr * dc + Mrr * dc * dc) / det) * I
            S0 = w.sum()
            if not np.isfinite(S0) or not S0 > 0.0:
                status = FAILED
                break
            mr, mc = (w * dr).sum() / S0, (w * dc).sum() / S0
            Nrr = 2.0 * ((w * dr * dr).sum() / S0 - mr * mr)
            Nrc = 2.0 * ((w * dr * dc).sum() / S0 - mr * mc)
            Ncc = 2.0 * ((w * dc * dc).sum() / S0 - mc * mc)
            step = 2.0 * max(abs(mr), abs(mc))
            tr = Nrr + Ncc
            dM = np.float64(max(abs(Nrr - Mrr), abs(Nrc - Mrc), abs(Ncc - Mcc))) / np.float64(tr)
            r0, c0 = r0 + 2.0 * mr, c0 + 2.0 * mc
            Mrr, Mrc, Mcc = Nrr, Nrc, Ncc
            if not abs(r0 - ctr) <= cs / 2.0 or not abs(c0 - ctr) <= cs / 2.0 or not (np.isfinite(tr) and tr >= 0.0):
                status = FAILED
                break
            if step < tol and dM < tol:
                status = CONVERGED
                break
    return np.array([r0, c0, Mrr, Mrc, Mcc], dtype=np.float64), it, status


def gauss(n, state):
    """g_X on an n x n grid: exp(-1/2 (x - x0)^T M^-1 (x - x0)) of state = (r0, c0, Mrr, Mrc, Mcc)"""
    r0, c0, Mrr, Mrc, Mcc = state
    det = Mrr * Mcc - Mrc * Mrc
    dr = np.arange(n, dtype=np.float64)[:, None] - r0
    dc = np.arange(n, dtype=np.float64)[None, :] - c0
    return np.exp(-0.5 * (Mcc * dr * dr - 2.0 * Mrc * dr * dc + Mrr * dc * dc) / det)


def rho4(I, state, status):
    """step 6: the kurtosis of I under the Gaussian of its final state"""
    if status == FAILED:
        return np.nan
    r0, c0, Mrr, Mrc, Mcc = state
    n = I.shape[0]
    det = Mrr * Mcc - Mrc * Mrc
    with np.errstate(all="ignore"):
        dr = np.arange(n, dtype=np.float64)[:, None] - r0
        dc = np.arange(n, dtype=np.float64)[None, :] - c0
        rho2 = (Mcc * dr * dr - 2.0 * Mrc * dr * dc + Mrr * dc * dc) / det
        w = np.exp(-0.5 * rho2) * I
        den = w.sum()
        return (w * rho2 * rho2).sum() / den if den > 0.0 else np.nan


def psf_row(Q, psf_sigma0=2.0, tol=1e-10, max_iter=200):
    """step 1 for one PSF image: dict(shape (5,), iters, status, aux (3,) = {A_P, FQ, rho4}, eps (ps, ps), usable)"""
    Q = np.asarray(Q, dtype=np.float64)
    ps = Q.shape[0]
    shape, it, st = mo.adaptive_moments(Q, psf_sigma0, tol, max_iter)
    FQ = Q.sum()
    det = shape[2] * shape[4] - shape[3] * shape[3]
    AP, k4, eps = np.nan, np.nan, np.full((ps, ps), np.nan)
    with np.errstate(all="ignore"):
        if st != FAILED and np.isfinite(det) and det > 1e-6:
            g = gauss(ps, shape)
            AP = (g * Q).sum() / (g * g).sum()
            k4 = rho4(Q, shape, st)
            eps = (Q - AP * g) / FQ
    usable = st == CONVERGED and np.isfinite(FQ) and FQ > 0.0 and np.isfinite(det) and det > 1e-6
    return dict(shape=shape, iters=it, status=st, aux=np.array([AP, FQ, k4]), eps=eps, usable=bool(usable))


def regauss_one(I, row, status, P, tol=1e-10, max_iter=200):
    """steps 2 - 6 for one band plane I (cs, cs) with its catalogue row (5,) and status, and its PSF row P (psf_row's
    dictionary, or None for an index out of range) -> ((r', c', Mrr', Mrc', Mcc', rho4), iters, status)"""
    nan6 = np.full(6, np.nan)
    I = np.asarray(I, dtype=np.float64)
    row = np.asarray(row, dtype=np.float64)
    cs = I.shape[0]
    r0, c0, Mrr, Mrc, Mcc = row
    with np.errstate(all="ignore"):
        detI = Mrr * Mcc - Mrc * Mrc
    if status not in (CONVERGED, ITER_LIMIT) or not np.all(np.isfinite(row)) or not (np.isfinite(detI) and detI > 1e-6):
        return nan6, 0, INELIGIBLE
    if P is None or not P["usable"]:
        return nan6, 0, NO_PSF
    q0r, q0c, Prr, Prc, Pcc = P["shape"]
    Zrr, Zrc, Zcc = Mrr - Prr, Mrc - Prc, Mcc - Pcc
    det0 = Zrr * Zcc - Zrc * Zrc
    if not Zrr > 0.0 or not (np.isfinite(det0) and det0 > 1e-6):
        return nan6, 0, UNRESOLVED
    gI = gauss(cs, row)
    AI = (gI * I).sum() / (gI * gI).sum()
    F0 = 2.0 * np.pi * np.sqrt(detI) * AI
    amp = F0 / (2.0 * np.pi * np.sqrt(det0))
    ps = P["eps"].shape[0]
    # f0 at x - (r0, c0) - (j - q0) for every stamp pixel x, one PSF pixel j at a time, in row-major order
    xr = np.arange(cs, dtype=np.float64)[:, None] - r0
    xc = np.arange(cs, dtype=np.float64)[None, :] - c0
    Ip = I.copy()
    corr = np.zeros((cs, cs))
    for jr in range(ps):
        dr = xr - (jr - q0r)
        for jc in range(ps):
            dc = xc - (jc - q0c)
            corr += P["eps"][jr, jc] * amp * np.exp(-0.5 * (Zcc * dr * dr - 2.0 * Zrc * dr * dc + Zrr * dc * dc) / det0)
    Ip -= corr
    state, it, st = adaptive_moments_from(Ip, row, tol, max_iter)
    return np.concatenate([state, [rho4(Ip, state, st)]]), it, st


def regauss(stamps, shape, status, psf_index, psf, band=2, psf_sigma0=2.0, tol=1e-10, max_iter=200):
    """the stamp-level call: dict(regauss (N, 6), regauss_iters, regauss_status, psf_shape (K, 5), psf_aux (K, 3), psf_iters,
    psf_status)"""
    stamps = np.asarray(stamps)
    psf = np.asarray(psf, dtype=np.float64)
    n, K = stamps.shape[0], psf.shape[0]
    rows = [psf_row(psf[k], psf_sigma0, tol, max_iter) for k in range(K)]
    out = dict(regauss=np.zeros((n, 6)), regauss_iters=np.zeros(n, np.int32), regauss_status=np.zeros(n, np.int32),
               psf_shape=np.array([p["shape"] for p in rows]).reshape(K, 5), psf_aux=np.array([p["aux"] for p in rows]).reshape(K, 3),
               psf_iters=np.array([p["iters"] for p in rows], np.int32), psf_status=np.array([p["status"] for p in rows], np.int32))
    for i in range(n):
        k = int(psf_index[i])
        P = rows[k] if 0 <= k < K else None
        out["regauss"][i], out["regauss_iters"][i], out["regauss_status"][i] = regauss_one(
            stamps[i, :, :, band].astype(np.float64), shape[i], int(status[i]), P, tol, max_iter)
    return out


def derived(regauss_rows, regauss_status, psf_shape, psf_index):
    """step 7: dict(sigma_corr, e1_corr, e2_corr, resolution), each (N,)"""
    R = np.asarray(regauss_rows, dtype=np.float64).reshape(-1, 6)
    n = R.shape[0]
    out = {k: np.full(n, np.nan) for k in ("sigma_corr", "e1_corr", "e2_corr", "resolution")}
    K = len(psf_shape)
    for i in range(n):
        k = int(psf_index[i])
        if regauss_status[i] >= FAILED or not 0 <= k < K:
            continue
        Prr, Prc, Pcc = psf_shape[k][2:5]
        Grr, Grc, Gcc = R[i, 2] - Prr, R[i, 3] - Prc, R[i, 4] - Pcc
        out["resolution"][i] = 1.0 - (Prr + Pcc) / (R[i, 2] + R[i, 4])
        det, tr = Grr * Gcc - Grc * Grc, Grr + Gcc
        if det > 0.0 and tr > 0.0:
            out["sigma_corr"][i] = det ** 0.25
            out["e1_corr"][i] = (Gcc - Grr) / tr
            out["e2_corr"][i] = 2.0 * Grc / tr
    return out


# ---- stamps of the test families -------------------------------------------------------------------------------------------
def cov(sigma, e1, e2):
    """(Mrr, Mrc, Mcc) of a Gaussian of size sigma = det^(1/4) and ellipticity e1 = (Mcc - Mrr) / tr, e2 = 2 Mrc / tr"""
    t = 2.0 * sigma * sigma / np.sqrt(1.0 - e1 * e1 - e2 * e2)
    return np.array([0.5 * t * (1.0 - e1), 0.5 * t * e2, 0.5 * t * (1.0 + e1)])


def norm_gaussian(n, M, offset, flux=1.0):
    """a Gaussian of total flux `flux` and covariance M centred at (n - 1) / 2 + offset, sampled at the pixel centres"""
    det = M[0] * M[2] - M[1] * M[1]
    return mo.gaussian_stamp(n, M, offset, flux / (2.0 * np.pi * np.sqrt(det)))


def double_gaussian_case(seed, cs=31, ps=21):
    """One case of the double-Gaussian family: a PSF of 0.85 core + 0.15 wing (the wing's covariance 4x the core's) and the
    exact image of a Gaussian galaxy seen through it.  Returns (stamp (cs, cs), psf (ps, ps), C_f (3,))."""
    rng = np.random.default_rng(seed)
    Cc = cov(rng.uniform(1.2, 1.6), rng.uniform(-0.08, 0.08), rng.uniform(-0.08, 0.08))
    Cf = cov(rng.uniform(1.5, 3.0), rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4))
    og, op = rng.uniform(-1.0, 1.0, 2), rng.uniform(-0.5, 0.5, 2)
    psf = 0.85 * norm_gaussian(ps, Cc, op) + 0.15 * norm_gaussian(ps, 4.0 * Cc, op)
    stamp = 0.85 * norm_gaussian(cs, Cf + Cc, og, 100.0) + 0.15 * norm_gaussian(cs, Cf + 4.0 * Cc, og, 100.0)
    return stamp, psf, Cf
