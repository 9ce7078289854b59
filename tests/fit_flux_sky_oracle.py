"""Numpy restatement of the flux fit with a sky background fitted jointly (csrc/fitflux.hip): the sums
E, K and c of step 1 in raster order with the sums of their absolute terms, the bordered matrix [[G, E], [E^T, K]], its solve -
tests/fit_flux_oracle.py's solve_band with the one change of the definition: a dropped sky term has amplitude 0 and leaves the
right-hand sides alone - and the chi-square of the weighted fit with the sky in the model.  G and h are the sums of
tests/fit_flux_oracle.py and tests/fit_flux_weighted_oracle.py, unchanged.  Float64, one field at a time."""
import numpy as np

from tests import fit_flux_oracle as fo
from tests import fit_flux_weighted_oracle as fw
from tests.fit_flux_oracle import _seq_sum, clip, gram_field, solve_band  # noqa: F401  (solve_band: the no-sky reference)


def sky_terms(order):
    return {0: 1, 1: 3}[order]


def basis(F, q):
    """B (F, F, q): B_0 = 1, B_1 = (2 r - F + 1) / F, B_2 = (2 c - F + 1) / F - an integer numerator, one division"""
    x = (2 * np.arange(F, dtype=np.int64) - F + 1).astype(np.float64) / np.float64(F)
    B = np.ones((F, F, q))
    if q == 3:
        B[:, :, 1] = x[:, None]
        B[:, :, 2] = x[None, :]
    return B


def field_sums(data, weight, q):
    """K, Kabs (nb, q, q) - the lower triangle, K_tu = sum (W B_t) B_u -, c, cabs (nb, q) with c_t = sum (W B_t) D, and npix (nb,)
    int64, over the counting pixels of the field (all of them with weight None), raster order"""
    F, nb = data.shape[0], data.shape[2]
    B = basis(F, q)
    K, Ka, c, ca = np.zeros((nb, q, q)), np.zeros((nb, q, q)), np.zeros((nb, q)), np.zeros((nb, q))
    npix = np.zeros(nb, np.int64)
    with np.errstate(all="ignore"):
        for b in range(nb):
            W = np.ones((F, F)) if weight is None else weight[:, :, b]
            on = np.ones((F, F), bool) if weight is None else fw.counts(W)
            npix[b] = int(on.sum())
            for t in range(q):
                wb = W * B[:, :, t]
                for u in range(t + 1):
                    terms = fw._select(on, wb * B[:, :, u])
                    K[b, t, u], Ka[b, t, u] = _seq_sum(terms), _seq_sum(np.abs(terms))
                terms = fw._select(on, wb * data[:, :, b])
                c[b, t], ca[b, t] = _seq_sum(terms), _seq_sum(np.abs(terms))
    return K, Ka, c, ca, npix


def border(stamps, places, F, weight, q):
    """E, Eabs (nb, n, q): E_it = sum over the pixels of galaxy i of (W P_i) B_t, raster order over the clipped stamp"""
    stamps = np.asarray(stamps, dtype=np.float32)
    n, cs, nb = stamps.shape[0], stamps.shape[1], stamps.shape[3]
    P = stamps.astype(np.float64)
    B = basis(F, q)
    E, Ea = np.zeros((nb, n, q)), np.zeros((nb, n, q))
    with np.errstate(all="ignore"):
        for i in range(n):
            ra, rz, ca, cz = clip(places[i], cs, F)
            if rz <= ra or cz <= ca:
                continue
            pi = P[i, ra - places[i][0]:rz - places[i][0], ca - places[i][1]:cz - places[i][1]]
            for b in range(nb):
                if weight is None:
                    wi, on = pi[:, :, b], np.ones(pi.shape[:2], bool)
                else:
                    wi, on = weight[ra:rz, ca:cz, b] * pi[:, :, b], fw.counts(weight[ra:rz, ca:cz, b])
                for t in range(q):
                    terms = fw._select(on, wi * B[ra:rz, ca:cz, t])
                    E[b, i, t], Ea[b, i, t] = _seq_sum(terms), _seq_sum(np.abs(terms))
    return E, Ea


def bordered(G, E, K):
    """The lower triangle (n + q, n + q) of [[G, E], [E^T, K]] of one band from the lower triangles G (n, n), K (q, q) and E (n, q)"""
    n, q = G.shape[0], K.shape[0]
    A = np.zeros((n + q, n + q))
    A[:n, :n] = np.tril(G)
    A[n:, :n] = E.T
    A[n:, n:] = np.tril(K)
    return A


def solve_band_sky(A, rhs, n, min_pivot=1e-8):
    """Steps 2 - 5 on the lower triangle A (n + q, n + q) and rhs (n + q,) of one band: solve_band on the bordered system, but an
    unknown from n on (a sky term) that is dropped has amplitude 0, and only the dropped GALAXIES leave the right-hand sides.
    Returns a dict: scale, var, status over all n + q unknowns, kept, hp, L, full, and cov (n + q, n + q): the inverse of the kept
    system, NaN in the rows and columns of unknowns that are not kept."""
    A = np.asarray(A, dtype=np.float64)
    nt = A.shape[0]
    full = np.tril(A) + np.tril(A, -1).T
    status = np.zeros(nt, np.int32)
    with np.errstate(all="ignore"):
        for i in range(nt):
            if not (np.isfinite(A[i, i]) and A[i, i] > 0.0):
                status[i] = 4
        L = np.zeros((nt, nt))
        kept = []
        for k in range(nt):
            if status[k]:
                continue
            d = A[k, k] - sum(L[k, j] * L[k, j] for j in kept)
            if d <= min_pivot * A[k, k]:
                status[k] = 5
                continue
            L[k, k] = np.sqrt(d)
            for i in range(k + 1, nt):
                if status[i] == 0:
                    L[i, k] = (A[i, k] - sum(L[i, j] * L[k, j] for j in kept)) / L[k, k]
            kept.append(k)
        kept = np.array(kept, dtype=np.int64)
        dropped = np.flatnonzero(status == 5)
        dropped_gal = dropped[dropped < n]
        scale, var = np.full(nt, np.nan), np.full(nt, np.nan)
        scale[dropped_gal] = 1.0
        scale[dropped[dropped >= n]] = 0.0
        hp = np.array([rhs[i] - sum(full[i, k] for k in dropped_gal) for i in kept], dtype=np.float64)
        Lk = L[np.ix_(kept, kept)]
        m = len(kept)
        y = np.zeros(m)
        for r in range(m):
            y[r] = (hp[r] - sum(Lk[r, c] * y[c] for c in range(r))) / Lk[r, r]
        a = np.zeros(m)
        for r in range(m - 1, -1, -1):
            a[r] = (y[r] - sum(Lk[c, r] * a[c] for c in range(r + 1, m))) / Lk[r, r]
        X = np.zeros((m, m))
        for i in range(m):
            X[i, i] = 1.0 / Lk[i, i]
            for r in range(i + 1, m):
                X[r, i] = -sum(Lk[r, c] * X[c, i] for c in range(i, r)) / Lk[r, r]
        scale[kept] = a
        var[kept] = (X * X).sum(axis=0)
        cov = np.full((nt, nt), np.nan)
        cov[np.ix_(kept, kept)] = X.T @ X
    return dict(scale=scale, var=var, status=status, kept=kept, hp=hp, L=Lk, full=full, cov=cov)


def chi2_field(stamps, places, data, weight, scale, status, sky_coef, sky_status):
    """Step 3 of one field on GIVEN amplitudes and sky: tests/fit_flux_weighted_oracle.py's chi2_field with sum_t s_t B_t(p) added
    to M behind the neighbours, t ascending, over the terms with sky_status 0 (sky_coef, sky_status (nb, q)).  Returns chi2,
    npix and yard = sum W R^2 with R = |D| + sum |a_j P_j| + sum |s_t B_t|."""
    stamps = np.asarray(stamps, dtype=np.float32)
    n, cs, nb = stamps.shape[0], stamps.shape[1], stamps.shape[3]
    F, q = data.shape[0], sky_coef.shape[1]
    P = stamps.astype(np.float64)
    Bf = basis(F, q)
    on = fw.counts(weight)
    chi2, yard = np.full((n, nb), np.nan), np.zeros((n, nb))
    npix = np.zeros((n, nb), np.int32)
    rects = [clip(places[i], cs, F) for i in range(n)]
    with np.errstate(all="ignore"):
        for i in range(n):
            ri = rects[i]
            if ri[1] <= ri[0] or ri[3] <= ri[2]:
                continue
            M = np.zeros((ri[1] - ri[0], ri[3] - ri[2], nb))
            A = np.zeros_like(M)
            for j in range(n):
                rj = rects[j]
                ra, rz, ca, cz = max(ri[0], rj[0]), min(ri[1], rj[1]), max(ri[2], rj[2]), min(ri[3], rj[3])
                if rz <= ra or cz <= ca:
                    continue
                pj = P[j, ra - places[j][0]:rz - places[j][0], ca - places[j][1]:cz - places[j][1]]
                sub = (slice(ra - ri[0], rz - ri[0]), slice(ca - ri[2], cz - ri[2]))
                for b in range(nb):
                    if status[j, b] != 4:
                        t = scale[j, b] * pj[:, :, b]
                        M[sub][:, :, b] = M[sub][:, :, b] + t
                        A[sub][:, :, b] = A[sub][:, :, b] + np.abs(t)
            D, W, o = data[ri[0]:ri[1], ri[2]:ri[3]], weight[ri[0]:ri[1], ri[2]:ri[3]], on[ri[0]:ri[1], ri[2]:ri[3]]
            B = Bf[ri[0]:ri[1], ri[2]:ri[3]]
            for b in range(nb):
                for t in range(q):
                    if sky_status[b, t] == 0:
                        term = sky_coef[b, t] * B[:, :, t]
                        M[:, :, b] = M[:, :, b] + term
                        A[:, :, b] = A[:, :, b] + np.abs(term)
                r = D[:, :, b] - M[:, :, b]
                npix[i, b] = int(o[:, :, b].sum())
                R = np.abs(D[:, :, b]) + A[:, :, b]
                yard[i, b] = _seq_sum(fw._select(o[:, :, b], (W[:, :, b] * R) * R))
                if status[i, b] != 4:
                    chi2[i, b] = _seq_sum(fw._select(o[:, :, b], (W[:, :, b] * r) * r))
    return chi2, npix, yard


def fit_flux_sky(stamps, places, field_ptr, data_fields, sky_order=0, weight_fields=None, min_pivot=1e-8, zero_coupling=False,
                 step1=None):
    """The outputs of dv_scene_fit_flux_sky: returns (out, fields).  out: the galaxy rows fit_scale, fit_var, fit_gram, fit_proj,
    fit_status (N, nb) (weighted: fit_chi2, fit_npix, chi2_yard too), gram_abs, proj_abs, and per field sky_coef (M, nb, q),
    sky_cov (M, nb, q, q), sky_status (M, nb, q), sky_npix (M, nb).  fields[m] = dict(A, Aabs (nb, n + q, n + q): the bordered
    lower triangles and the sums of their absolute terms; rhs, rhsabs (n + q, nb); bands=[solve_band_sky]).  zero_coupling: E
    is set to 0 by hand - the galaxy rows are then those of the fit without sky.  step1: per field the dict(G, Gabs, h, habs)
    that fit_flux of tests/fit_flux_oracle.py (weighted: of tests/fit_flux_weighted_oracle.py) returned for the same scene, to
    spare computing those sums again."""
    stamps = np.asarray(stamps, dtype=np.float32)
    N, nb = stamps.shape[0], stamps.shape[3]
    places = np.asarray(places, dtype=np.int64).reshape(N, 2)
    fp = np.asarray(field_ptr, dtype=np.int64)
    M, q = len(fp) - 1, sky_terms(sky_order)
    out = {k: np.zeros((N, nb)) for k in ("fit_scale", "fit_var", "fit_gram", "fit_proj", "gram_abs", "proj_abs")}
    out["fit_status"] = np.zeros((N, nb), np.int32)
    if weight_fields is not None:
        out["fit_chi2"], out["chi2_yard"], out["fit_npix"] = np.zeros((N, nb)), np.zeros((N, nb)), np.zeros((N, nb), np.int32)
    out.update(sky_coef=np.zeros((M, nb, q)), sky_cov=np.zeros((M, nb, q, q)), sky_status=np.zeros((M, nb, q), np.int32),
               sky_npix=np.zeros((M, nb), np.int64))
    fields = []
    for m in range(M):
        lo, hi = int(fp[m]), int(fp[m + 1])
        n = hi - lo
        D = np.asarray(data_fields[m], dtype=np.float64)
        W = None if weight_fields is None else np.asarray(weight_fields[m], dtype=np.float64)
        F = D.shape[0]
        if step1 is not None:
            G, Ga, h, ha = (step1[m][k] for k in ("G", "Gabs", "h", "habs"))
            gnpix = None
        elif W is None:
            G, Ga, h, ha = gram_field(stamps[lo:hi], places[lo:hi], D)
        else:
            G, Ga, h, ha, gnpix = fw.gram_field(stamps[lo:hi], places[lo:hi], D, W)
        E, Ea = border(stamps[lo:hi], places[lo:hi], F, W, q)
        if zero_coupling:
            E = np.zeros_like(E)
        K, Ka, c, ca, npix = field_sums(D, W, q)
        A = np.stack([bordered(G[b], E[b], K[b]) for b in range(nb)]) if nb else np.zeros((0, n + q, n + q))
        Aa = np.stack([bordered(Ga[b], Ea[b], Ka[b]) for b in range(nb)])
        rhs, rhsa = np.concatenate([h, c.T]), np.concatenate([ha, ca.T])
        bands = [solve_band_sky(A[b], rhs[:, b], n, min_pivot) for b in range(nb)]
        for b, s in enumerate(bands):
            out["fit_scale"][lo:hi, b], out["fit_var"][lo:hi, b] = s["scale"][:n], s["var"][:n]
            out["fit_status"][lo:hi, b] = s["status"][:n]
            out["fit_gram"][lo:hi, b], out["gram_abs"][lo:hi, b] = np.diagonal(G[b]), np.diagonal(Ga[b])
            out["sky_coef"][m, b], out["sky_status"][m, b] = s["scale"][n:], s["status"][n:]
            out["sky_cov"][m, b] = s["cov"][n:, n:]
        out["fit_proj"][lo:hi], out["proj_abs"][lo:hi] = h, ha
        out["sky_npix"][m] = npix
        if W is not None:
            chi2, npix2, yard = chi2_field(stamps[lo:hi], places[lo:hi], D, W, out["fit_scale"][lo:hi], out["fit_status"][lo:hi],
                                           out["sky_coef"][m], out["sky_status"][m])
            assert gnpix is None or np.array_equal(gnpix, npix2)
            out["fit_chi2"][lo:hi], out["fit_npix"][lo:hi], out["chi2_yard"][lo:hi] = chi2, npix2, yard
        fields.append(dict(A=A, Aabs=Aa, rhs=rhs, rhsabs=rhsa, bands=bands))
    return out, fields


def scaled_condition(full, kept):
    """fit_flux_oracle.scaled_condition on the bordered matrix"""
    return fo.scaled_condition(full, kept)
