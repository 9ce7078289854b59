"""Numpy restatement of the simultaneous flux fit (csrc/fitflux.hip): steps 1 - 5 of the definition,
float64, one field and one band at a time.  The sums of step 1 run in raster order over the intersection of the two clipped
stamps and come with the sums of their absolute terms, the yardstick of the GPU comparison (a sum of N terms in any order
differs from another order by at most N 2^-53 times the sum of the absolute terms).  The factorisation is the textbook
left-looking Cholesky with the dropping rule of the definition; its order of additions is not the kernel's, which the GPU
tests allow for with bounds derived from the condition number."""
import numpy as np


def _seq_sum(x):
    """The sum of x in the order given, rounded after every addition"""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    return float(np.cumsum(x)[-1]) if x.size else 0.0


def clip(place, cs, F):
    """The field rows and columns [ra, rz) x [ca, cz) a stamp at `place` covers inside the field (empty: rz <= ra or cz <= ca)"""
    pr, pc = int(place[0]), int(place[1])
    return max(pr, 0), min(pr + cs, F), max(pc, 0), min(pc + cs, F)


def gram_field(stamps, places, data):
    """Step 1 for the n galaxies of one field: stamps (n, cs, cs, nb) float32, places (n, 2), data (F, F, nb).  Returns G, Gabs
    (nb, n, n) - the lower triangle, exactly 0.0 above the diagonal and where two clipped rectangles do not intersect - and h,
    habs (n, nb)."""
    stamps = np.asarray(stamps, dtype=np.float32)
    n, cs, nb = stamps.shape[0], stamps.shape[1], stamps.shape[3]
    F = data.shape[0]
    P = stamps.astype(np.float64)
    G, Ga = np.zeros((nb, n, n)), np.zeros((nb, n, n))
    h, ha = np.zeros((n, nb)), np.zeros((n, nb))
    for i in range(n):
        ri = clip(places[i], cs, F)
        for j in range(i + 1):
            rj = clip(places[j], cs, F)
            ra, rz, ca, cz = max(ri[0], rj[0]), min(ri[1], rj[1]), max(ri[2], rj[2]), min(ri[3], rj[3])
            if rz <= ra or cz <= ca:
                continue
            pi = P[i, ra - places[i][0]:rz - places[i][0], ca - places[i][1]:cz - places[i][1]]
            pj = P[j, ra - places[j][0]:rz - places[j][0], ca - places[j][1]:cz - places[j][1]]
            for b in range(nb):
                t = pi[:, :, b] * pj[:, :, b]
                G[b, i, j], Ga[b, i, j] = _seq_sum(t), _seq_sum(np.abs(t))
                if i == j:
                    t = pi[:, :, b] * data[ra:rz, ca:cz, b]
                    h[i, b], ha[i, b] = _seq_sum(t), _seq_sum(np.abs(t))
    return G, Ga, h, ha


def solve_band(G, h, min_pivot=1e-8):
    """Steps 2 - 5 on the lower triangle G (n, n) and h (n,) of one band.  Returns a dict: scale, var (n,), status (n,) int32,
    kept (the indices of the fitted galaxies, ascending), hp (the right-hand side of the kept system, step 4) and L (its
    Cholesky factor)."""
    G = np.asarray(G, dtype=np.float64)
    n = G.shape[0]
    full = np.tril(G) + np.tril(G, -1).T
    status = np.zeros(n, np.int32)
    with np.errstate(all="ignore"):
        for i in range(n):
            if not (np.isfinite(G[i, i]) and G[i, i] > 0.0):
                status[i] = 4
        L = np.zeros((n, n))
        kept = []
        for k in range(n):
            if status[k]:
                continue
            d = G[k, k] - sum(L[k, j] * L[k, j] for j in kept)
            if d <= min_pivot * G[k, k]:
                status[k] = 5                                 # dropped: never applied to the others
                continue
            L[k, k] = np.sqrt(d)
            for i in range(k + 1, n):
                if status[i] == 0:
                    L[i, k] = (G[i, k] - sum(L[i, j] * L[k, j] for j in kept)) / L[k, k]
            kept.append(k)
        kept = np.array(kept, dtype=np.int64)
        dropped = np.flatnonzero(status == 5)
        scale, var = np.full(n, np.nan), np.full(n, np.nan)
        scale[dropped] = 1.0
        hp = np.array([h[i] - sum(full[i, k] for k in dropped) for i in kept], dtype=np.float64)
        Lk = L[np.ix_(kept, kept)]
        m = len(kept)
        y = np.zeros(m)
        for r in range(m):
            y[r] = (hp[r] - sum(Lk[r, c] * y[c] for c in range(r))) / Lk[r, r]
        a = np.zeros(m)
        for r in range(m - 1, -1, -1):
            a[r] = (y[r] - sum(Lk[c, r] * a[c] for c in range(r + 1, m))) / Lk[r, r]
        X = np.zeros((m, m))                                  # L^-1, column by column
        for i in range(m):
            X[i, i] = 1.0 / Lk[i, i]
            for r in range(i + 1, m):
                X[r, i] = -sum(Lk[r, c] * X[c, i] for c in range(i, r)) / Lk[r, r]
        scale[kept] = a
        var[kept] = (X * X).sum(axis=0)
    return dict(scale=scale, var=var, status=status, kept=kept, hp=hp, L=Lk, full=full)


def fit_flux(stamps, places, field_ptr, data_fields, min_pivot=1e-8):
    """The five outputs of dv_scene_fit_flux, (N, nb) each, plus per field the step-1 sums and per (field, band) the solve:
    returns (out, fields) with out = {fit_scale, fit_var, fit_gram, fit_proj, fit_status, gram_abs, proj_abs} and fields[m] =
    dict(G, Gabs, h, habs, bands=[solve_band(...)])."""
    stamps = np.asarray(stamps, dtype=np.float32)
    N, nb = stamps.shape[0], stamps.shape[3]
    places = np.asarray(places, dtype=np.int64).reshape(N, 2)
    fp = np.asarray(field_ptr, dtype=np.int64)
    out = dict(fit_scale=np.zeros((N, nb)), fit_var=np.zeros((N, nb)), fit_gram=np.zeros((N, nb)), fit_proj=np.zeros((N, nb)),
               fit_status=np.zeros((N, nb), np.int32), gram_abs=np.zeros((N, nb)), proj_abs=np.zeros((N, nb)))
    fields = []
    for m in range(len(fp) - 1):
        lo, hi = int(fp[m]), int(fp[m + 1])
        G, Ga, h, ha = gram_field(stamps[lo:hi], places[lo:hi], np.asarray(data_fields[m], dtype=np.float64))
        bands = [solve_band(G[b], h[:, b], min_pivot) for b in range(nb)]
        for b, s in enumerate(bands):
            out["fit_scale"][lo:hi, b], out["fit_var"][lo:hi, b], out["fit_status"][lo:hi, b] = s["scale"], s["var"], s["status"]
            out["fit_gram"][lo:hi, b] = np.diagonal(G[b])
            out["gram_abs"][lo:hi, b] = np.diagonal(Ga[b])
        out["fit_proj"][lo:hi], out["proj_abs"][lo:hi] = h, ha
        fields.append(dict(G=G, Gabs=Ga, h=h, habs=ha, bands=bands))
    return out, fields


def scaled_condition(full, kept):
    """The 2-norm condition number of the kept Gram matrix scaled to a unit diagonal (1.0 for an empty or 1 x 1 system)"""
    if len(kept) < 2:
        return 1.0
    A = full[np.ix_(kept, kept)]
    d = 1.0 / np.sqrt(np.diagonal(A))
    return float(np.linalg.cond(A * d[:, None] * d[None, :]))


def elliptical_gaussian(cs, M, offset=(0.0, 0.0), amp=1.0):
    """amp * exp(-1/2 x^T M^-1 x) on a cs x cs stamp about its centre + offset, M = (Mrr, Mrc, Mcc); float64 (cs, cs)"""
    Mrr, Mrc, Mcc = M
    det = Mrr * Mcc - Mrc * Mrc
    ctr = (cs - 1) / 2.0
    r = np.arange(cs, dtype=np.float64)[:, None] - ctr - offset[0]
    c = np.arange(cs, dtype=np.float64)[None, :] - ctr - offset[1]
    return amp * np.exp(-0.5 * (Mcc * r * r - 2.0 * Mrc * r * c + Mrr * c * c) / det)
