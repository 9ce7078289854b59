"""Numpy restatement of the weighted flux fit (csrc/fitflux.hip): step 1 with per-pixel weights and
masks, and step 3, the chi-square of the refitted scene; steps 2 - 5 of the solve are tests/fit_flux_oracle.py's, unchanged.
Float64, one field at a time.  A pixel of band b counts iff 0 < W < inf; every other pixel's terms are +0.0 by selection
(numpy.where), so a NaN under a masked pixel reaches no sum.  Sums run in raster order and come with the sums of their absolute
terms.  The chi-square takes fit_scale and fit_status as inputs, so the GPU's chi-square can be compared on the GPU's own
amplitudes without the solve's rounding in between; it also returns sum W R^2 with R = |D| + sum |a_j P_j|, the yardstick of
that comparison: every rounding of M, of r and of the terms is a multiple of 2^-53 of a quantity bounded by R or W R^2."""
import numpy as np

from tests.fit_flux_oracle import _seq_sum, clip, solve_band


def counts(W):
    """where a pixel counts: 0 < W < inf (False for zero, negative, infinite and NaN weights)"""
    W = np.asarray(W, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (W > 0.0) & (W < np.inf)


def _select(on, terms):
    """the terms where `on`, exactly +0.0 elsewhere - whatever stands there"""
    return np.where(on, terms, 0.0)


def gram_field(stamps, places, data, weight):
    """Step 1 for the n galaxies of one field: stamps (n, cs, cs, nb) float32, places (n, 2), data and weight (F, F, nb).
    Returns G, Gabs (nb, n, n) - the lower triangle, G_ij = sum (W P_i) P_j over the counting pixels both stamps cover, exactly
    0.0 above the diagonal and where two clipped rectangles do not intersect -, h, habs (n, nb) with h_i = sum (W P_i) D, and
    npix (n, nb) int32, the counting pixels of every galaxy."""
    stamps = np.asarray(stamps, dtype=np.float32)
    n, cs, nb = stamps.shape[0], stamps.shape[1], stamps.shape[3]
    F = data.shape[0]
    P = stamps.astype(np.float64)
    on = counts(weight)
    G, Ga = np.zeros((nb, n, n)), np.zeros((nb, n, n))
    h, ha = np.zeros((n, nb)), np.zeros((n, nb))
    npix = np.zeros((n, nb), np.int32)
    with np.errstate(all="ignore"):
        for i in range(n):
            ri = clip(places[i], cs, F)
            for j in range(i + 1):
                rj = clip(places[j], cs, F)
                ra, rz, ca, cz = max(ri[0], rj[0]), min(ri[1], rj[1]), max(ri[2], rj[2]), min(ri[3], rj[3])
                if rz <= ra or cz <= ca:
                    continue
                pi = P[i, ra - places[i][0]:rz - places[i][0], ca - places[i][1]:cz - places[i][1]]
                pj = P[j, ra - places[j][0]:rz - places[j][0], ca - places[j][1]:cz - places[j][1]]
                w, o = weight[ra:rz, ca:cz], on[ra:rz, ca:cz]
                for b in range(nb):
                    wi = w[:, :, b] * pi[:, :, b]                          # (the product with W first)
                    t = _select(o[:, :, b], wi * pj[:, :, b])
                    G[b, i, j], Ga[b, i, j] = _seq_sum(t), _seq_sum(np.abs(t))
                    if i == j:
                        t = _select(o[:, :, b], wi * data[ra:rz, ca:cz, b])
                        h[i, b], ha[i, b] = _seq_sum(t), _seq_sum(np.abs(t))
                        npix[i, b] = int(o[:, :, b].sum())
    return G, Ga, h, ha, npix


def chi2_field(stamps, places, data, weight, scale, status):
    """Step 3 for the n galaxies of one field on GIVEN amplitudes: scale (n, nb) and status (n, nb) as the solve returned
    them.  Per galaxy i, band b and pixel p of i: M(p) = sum_j a_j P_j(p) over the galaxies j in ascending order that cover p
    and do not have status 4, added one after another from 0.0; r = D - M; chi2 = sum over the counting pixels of (W r) r in
    raster order, NaN where status[i, b] is 4.  Returns chi2 (n, nb), npix (n, nb) int32 and yard (n, nb) = sum over the
    counting pixels of W R^2, R = |D| + sum_j |a_j P_j|."""
    stamps = np.asarray(stamps, dtype=np.float32)
    n, cs, nb = stamps.shape[0], stamps.shape[1], stamps.shape[3]
    F = data.shape[0]
    P = stamps.astype(np.float64)
    on = counts(weight)
    scale, status = np.asarray(scale, dtype=np.float64), np.asarray(status)
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
            for b in range(nb):
                r = D[:, :, b] - M[:, :, b]
                npix[i, b] = int(o[:, :, b].sum())
                R = np.abs(D[:, :, b]) + A[:, :, b]
                yard[i, b] = _seq_sum(_select(o[:, :, b], (W[:, :, b] * R) * R))
                if status[i, b] != 4:
                    chi2[i, b] = _seq_sum(_select(o[:, :, b], (W[:, :, b] * r) * r))
    return chi2, npix, yard


def fit_flux(stamps, places, field_ptr, data_fields, weight_fields, min_pivot=1e-8):
    """The seven outputs of dv_scene_fit_flux_weighted, (N, nb) each, plus the sums of the absolute terms and per field the
    step-1 sums and per (field, band) the solve: returns (out, fields) with out = {fit_scale, fit_var, fit_gram, fit_proj,
    fit_status, fit_chi2, fit_npix, gram_abs, proj_abs, chi2_yard} and fields[m] = dict(G, Gabs, h, habs, bands=[solve_band])."""
    stamps = np.asarray(stamps, dtype=np.float32)
    N, nb = stamps.shape[0], stamps.shape[3]
    places = np.asarray(places, dtype=np.int64).reshape(N, 2)
    fp = np.asarray(field_ptr, dtype=np.int64)
    out = {k: np.zeros((N, nb)) for k in ("fit_scale", "fit_var", "fit_gram", "fit_proj", "fit_chi2", "gram_abs", "proj_abs",
                                          "chi2_yard")}
    out["fit_status"], out["fit_npix"] = np.zeros((N, nb), np.int32), np.zeros((N, nb), np.int32)
    fields = []
    for m in range(len(fp) - 1):
        lo, hi = int(fp[m]), int(fp[m + 1])
        D, W = np.asarray(data_fields[m], dtype=np.float64), np.asarray(weight_fields[m], dtype=np.float64)
        G, Ga, h, ha, npix = gram_field(stamps[lo:hi], places[lo:hi], D, W)
        bands = [solve_band(G[b], h[:, b], min_pivot) for b in range(nb)]
        for b, s in enumerate(bands):
            out["fit_scale"][lo:hi, b], out["fit_var"][lo:hi, b], out["fit_status"][lo:hi, b] = s["scale"], s["var"], s["status"]
            out["fit_gram"][lo:hi, b] = np.diagonal(G[b])
            out["gram_abs"][lo:hi, b] = np.diagonal(Ga[b])
        out["fit_proj"][lo:hi], out["proj_abs"][lo:hi] = h, ha
        chi2, npix2, yard = chi2_field(stamps[lo:hi], places[lo:hi], D, W, out["fit_scale"][lo:hi], out["fit_status"][lo:hi])
        assert np.array_equal(npix, npix2)
        out["fit_chi2"][lo:hi], out["fit_npix"][lo:hi], out["chi2_yard"][lo:hi] = chi2, npix, yard
        fields.append(dict(G=G, Gabs=Ga, h=h, habs=ha, bands=bands))
    return out, fields
