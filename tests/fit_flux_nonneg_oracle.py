"""Numpy restatement of the non-negative flux fit (csrc/fitflux.hip): the iteration on the active set -
block principal pivoting (Kim & Park) with Murty's single exchange as the backup rule - around the solve of
tests/fit_flux_sky_oracle.py.  Iteration 1 IS solve_band_sky (with no sky term, solve_band): its statuses, dropped set, h' and
amplitudes are taken from it unchanged, so an all-positive system returns that function's arrays.  Later iterations factorise
the kept unknowns that are not clamped with the same left-looking Cholesky, without a pivot test.  Float64, one field and band
at a time.  Step 1 - G, E, K, h, c - is that of the three earlier restatements, unchanged."""
import numpy as np

from tests import fit_flux_oracle as fo
from tests import fit_flux_sky_oracle as fs
from tests import fit_flux_weighted_oracle as fw


def _cholesky(A):
    """The left-looking Cholesky factor of the dense symmetric A (no pivot test), as solve_band builds it"""
    m = A.shape[0]
    L = np.zeros((m, m))
    for k in range(m):
        L[k, k] = np.sqrt(A[k, k] - sum(L[k, j] * L[k, j] for j in range(k)))
        for i in range(k + 1, m):
            L[i, k] = (A[i, k] - sum(L[i, j] * L[k, j] for j in range(k))) / L[k, k]
    return L


def _solve(L, hp):
    """L y = hp, then L^T a = y, row by row as solve_band does"""
    m = L.shape[0]
    y = np.zeros(m)
    for r in range(m):
        y[r] = (hp[r] - sum(L[r, c] * y[c] for c in range(r))) / L[r, r]
    a = np.zeros(m)
    for r in range(m - 1, -1, -1):
        a[r] = (y[r] - sum(L[c, r] * a[c] for c in range(r + 1, m))) / L[r, r]
    return a


def _inverse(L):
    """X = L^-1, column by column as solve_band does"""
    m = L.shape[0]
    X = np.zeros((m, m))
    for i in range(m):
        X[i, i] = 1.0 / L[i, i]
        for r in range(i + 1, m):
            X[r, i] = -sum(L[r, c] * X[c, i] for c in range(i, r)) / L[r, r]
    return X


def first_iteration(A, rhs, n, min_pivot=1e-8, fast=False):
    """Iteration 1: solve_band_sky's dict.  fast (the systems of several hundred unknowns, which the loops above do not serve):
    numpy.linalg on a system that must have neither an ineligible nor a dropped unknown - asserted."""
    if not fast:
        return fs.solve_band_sky(A, rhs, n, min_pivot)
    A = np.asarray(A, dtype=np.float64)
    nt = A.shape[0]
    full = np.tril(A) + np.tril(A, -1).T
    d = np.diagonal(full)
    assert (np.isfinite(d) & (d > 0.0)).all()
    L = np.linalg.cholesky(full)
    assert (np.diagonal(L) ** 2 > 1e3 * min_pivot * d).all()            # (far from the dropping rule: no status 5)
    kept = np.arange(nt)
    return dict(scale=np.linalg.solve(full, rhs), status=np.zeros(nt, np.int32), kept=kept,
                hp=np.asarray(rhs, dtype=np.float64).copy(), full=full)


def solve_band_nonneg(A, rhs, n, min_pivot=1e-8, max_iter=100, fast=False):
    """The iteration of section 7u on the lower triangle A (n + q, n + q) and rhs (n + q,) of one band, the first n unknowns
    galaxies, the others sky terms.  Returns a dict over all n + q unknowns: scale (clamped: +0.0), var, status, free (the
    amplitudes of iteration 1), clamped (int32), dual (y_i where clamped, +0.0 where passive, NaN for status 4 or 5), cov (the
    inverse of the last passive system, NaN elsewhere), and kept, passive (indices), hp (over kept), full, iters, nn_status, and
    sizes: |V| of every iteration."""
    assert max_iter >= 1
    s0 = first_iteration(A, rhs, n, min_pivot, fast)
    nt, full, kept, status = len(s0["scale"]), s0["full"], s0["kept"], s0["status"]
    hp = np.full(nt, np.nan)
    hp[kept] = s0["hp"]
    free = s0["scale"].copy()
    Z = np.zeros(nt, bool)
    a = np.zeros(nt)
    a[kept] = free[kept]
    y = np.zeros(nt)
    best, p, sizes = n + 1, 3, []
    t = 1
    with np.errstate(all="ignore"):
        while True:
            P = kept[~Z[kept]]
            if t > 1:
                sub = full[np.ix_(P, P)]
                a[:] = 0.0
                if fast:
                    a[P] = np.linalg.solve(sub, hp[P]) if len(P) else []
                else:
                    a[P] = _solve(_cholesky(sub), hp[P])
            y[:] = 0.0
            for i in np.flatnonzero(Z):
                acc = 0.0
                for j in P:                                            # ascending, one addition after another
                    acc = acc + full[i, j] * a[j]
                y[i] = acc - hp[i]
            gal = np.arange(nt) < n
            V = np.flatnonzero((gal & ~Z & (status == 0) & (a < 0.0)) | (Z & (y < 0.0)))
            sizes.append(len(V))
            if len(V) == 0 or t >= max_iter:
                break
            if len(V) < best:
                best, p = len(V), 3
                Z[V] = ~Z[V]
            elif p > 0:
                p -= 1
                Z[V] = ~Z[V]
            else:
                Z[V[-1]] = ~Z[V[-1]]
            t += 1
        P = kept[~Z[kept]]
        sub = full[np.ix_(P, P)]
        var, cov = np.full(nt, np.nan), np.full((nt, nt), np.nan)
        if fast:
            inv = np.linalg.inv(sub) if len(P) else np.zeros((0, 0))
            var[P] = np.diagonal(inv)
            cov[np.ix_(P, P)] = inv
        elif t == 1:                                                   # the unconstrained fit was feasible: its arrays
            var, cov = s0["var"].copy(), s0["cov"].copy()
        else:
            X = _inverse(_cholesky(sub))
            var[P] = (X * X).sum(axis=0)
            cov[np.ix_(P, P)] = X.T @ X
    scale = s0["scale"].copy()                                         # (1 where dropped, 0 for a dropped sky term, NaN for 4)
    scale[P] = a[P]
    scale[Z] = 0.0
    dual = np.full(nt, np.nan)
    dual[status == 0] = 0.0
    dual[Z] = y[Z]
    return dict(scale=scale, var=var, status=status, free=free, clamped=Z.astype(np.int32), dual=dual, cov=cov, kept=kept,
                passive=P, hp=hp[kept], full=full, iters=t, nn_status=int(len(V) > 0), sizes=sizes)


def fit_flux_nonneg(stamps, places, field_ptr, data_fields, sky_order=None, weight_fields=None, min_pivot=1e-8, max_iter=100,
                    step1=None):
    """The outputs of dv_scene_fit_flux_nonneg: returns (out, fields).  out: the arrays of the call without the constraint as
    tests/fit_flux_oracle.py, tests/fit_flux_weighted_oracle.py or tests/fit_flux_sky_oracle.py return them (sky_order None: no
    sky) with fit_scale, fit_var, the sky arrays and the chi-square of the constrained fit, plus fit_scale_free, fit_clamped,
    fit_dual (N, nb) and nonneg_iters, nonneg_status (M, nb).  fields[m] = dict(A (nb, n + q, n + q), rhs (n + q, nb),
    bands=[solve_band_nonneg]).  step1: see fit_flux_sky."""
    stamps = np.asarray(stamps, dtype=np.float32)
    N, nb = stamps.shape[0], stamps.shape[3]
    places = np.asarray(places, dtype=np.int64).reshape(N, 2)
    fp = np.asarray(field_ptr, dtype=np.int64)
    M = len(fp) - 1
    q = 0 if sky_order is None else fs.sky_terms(sky_order)
    if sky_order is not None:
        out, base = fs.fit_flux_sky(stamps, places, fp, data_fields, sky_order, weight_fields, min_pivot, step1=step1)
        systems = [(f["A"], f["rhs"]) for f in base]
    else:
        if step1 is not None:
            base = step1
        elif weight_fields is None:
            base = fo.fit_flux(stamps, places, fp, data_fields, min_pivot)[1]
        else:
            base = fw.fit_flux(stamps, places, fp, data_fields, weight_fields, min_pivot)[1]
        systems = [(f["G"], f["h"]) for f in base]
        out = {k: np.zeros((N, nb)) for k in ("fit_scale", "fit_var", "fit_gram", "fit_proj", "gram_abs", "proj_abs")}
        out["fit_status"] = np.zeros((N, nb), np.int32)
        for m, f in enumerate(base):
            lo, hi = int(fp[m]), int(fp[m + 1])
            out["fit_gram"][lo:hi] = np.diagonal(f["G"], axis1=1, axis2=2).T
            out["gram_abs"][lo:hi] = np.diagonal(f["Gabs"], axis1=1, axis2=2).T
            out["fit_proj"][lo:hi], out["proj_abs"][lo:hi] = f["h"], f["habs"]
        if weight_fields is not None:
            out["fit_chi2"], out["chi2_yard"], out["fit_npix"] = np.zeros((N, nb)), np.zeros((N, nb)), np.zeros((N, nb), np.int32)
    out = {k: np.array(v) for k, v in out.items()}
    out.update(fit_scale_free=np.zeros((N, nb)), fit_clamped=np.zeros((N, nb), np.int32), fit_dual=np.zeros((N, nb)),
               nonneg_iters=np.zeros((M, nb), np.int32), nonneg_status=np.zeros((M, nb), np.int32))
    fields = []
    for m, (A, rhs) in enumerate(systems):
        lo, hi = int(fp[m]), int(fp[m + 1])
        n = hi - lo
        bands = [solve_band_nonneg(A[b], rhs[:, b], n, min_pivot, max_iter) for b in range(nb)] if n + q else []
        for b, s in enumerate(bands):
            for k, v in (("fit_scale", "scale"), ("fit_var", "var"), ("fit_status", "status"), ("fit_scale_free", "free"),
                         ("fit_clamped", "clamped"), ("fit_dual", "dual")):
                out[k][lo:hi, b] = s[v][:n]
            out["nonneg_iters"][m, b], out["nonneg_status"][m, b] = s["iters"], s["nn_status"]
            if q:
                out["sky_coef"][m, b], out["sky_status"][m, b], out["sky_cov"][m, b] = s["scale"][n:], s["status"][n:], s["cov"][n:, n:]
        if weight_fields is not None:
            D, W = np.asarray(data_fields[m], dtype=np.float64), np.asarray(weight_fields[m], dtype=np.float64)
            coef = out["sky_coef"][m] if q else np.zeros((nb, 0))
            stat = out["sky_status"][m] if q else np.zeros((nb, 0), np.int32)
            chi2, npix, yard = fs.chi2_field(stamps[lo:hi], places[lo:hi], D, W, out["fit_scale"][lo:hi], out["fit_status"][lo:hi],
                                             coef, stat)
            out["fit_chi2"][lo:hi], out["fit_npix"][lo:hi], out["chi2_yard"][lo:hi] = chi2, npix, yard
        fields.append(dict(A=A, rhs=rhs, bands=bands))
    return out, fields


def margins(s, n):
    """The three conditions under which rounding cannot move a set membership of the solve `s`: the scaled
    condition number of the kept system, the smallest a_i sqrt(G_ii) of a passive galaxy over max |a sqrt(G)|, the smallest
    y_i / sqrt(G_ii) of a clamped one over max |h' / sqrt(G)| (inf where there is none)"""
    full, kept, P = s["full"], s["kept"], s["passive"]
    g = np.sqrt(np.diagonal(full))
    cond = fo.scaled_condition(full, kept)
    Pg = P[P < n]
    sa = np.abs(s["scale"][P] * g[P]).max() if len(P) else 1.0
    passive = float((s["scale"][Pg] * g[Pg]).min() / sa) if len(Pg) else np.inf
    Z = np.flatnonzero(s["clamped"])
    hp = np.zeros(len(g))
    hp[kept] = s["hp"]
    sh = np.abs(hp[kept] / g[kept]).max() if len(kept) else 1.0
    clamped = float((s["dual"][Z] / g[Z]).min() / sh) if len(Z) else np.inf
    return cond, passive, clamped
