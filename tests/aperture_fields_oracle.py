"""numpy float64 restatement of the apertures on the fields: the sums of n T, n D and n over the stamp
pixels of positive sub-pixel count that lie inside the field, for the circles and the automatic ellipse of the aperture
photometry.  Written from the specification, not from the kernel; it is the reference of
tests/test_aperture_fields_host.py and tests/test_gpu_aperture_fields.py.  The regions, the counts and the sub-pixel offsets
are those of tests/aperture_oracle.py, imported rather than restated; the sums run in raster order over the stamp.  Beside
the outputs a row reports the absolute sums (sum n |x|) / s^2 the comparison bounds scale with."""
import numpy as np

from tests.aperture_oracle import INELIGIBLE, NO_KRON, OK, counts, offsets, params, quad, rsum  # noqa: F401

KEYS = ("ap_model_sum", "ap_data_sum", "ap_field_area", "auto_model_sum", "auto_data_sum", "auto_field_area")


def _region(T, D, cnt, place, F, s):
    """(model (nb,), data (nb,) or NaN, area, model_abs, data_abs) of one region: over the stamp pixels (r, c) with cnt > 0
    whose field pixel (pr + r, pc + c) lies inside the field, in raster order"""
    cs, nb = cnt.shape[0], T.shape[2]
    pr, pc = int(place[0]), int(place[1])
    rr, cc = np.nonzero(cnt > 0)                              # raster order
    fr, fc = rr + pr, cc + pc
    keep = (fr >= 0) & (fr < F) & (fc >= 0) & (fc < F)
    rr, cc, fr, fc = rr[keep], cc[keep], fr[keep], fc[keep]
    ws, s2 = cnt[rr, cc].astype(np.float64), np.float64(s * s)
    nan = np.full(nb, np.nan)
    model = np.array([rsum(ws * T[fr, fc, b]) for b in range(nb)]) / s2
    mabs = np.array([rsum(ws * np.abs(T[fr, fc, b])) for b in range(nb)]) / s2
    if D is None:
        data, dabs = nan, nan
    else:
        data = np.array([rsum(ws * D[fr, fc, b]) for b in range(nb)]) / s2
        dabs = np.array([rsum(ws * np.abs(D[fr, fc, b])) for b in range(nb)]) / s2
    return model, data, rsum(ws) / s2, mabs, dabs


def field_row(shape, status, aper_status, rho_auto, place, T, D, cs, par=None, shortcut=False):
    """One galaxy: shape = (r0, c0, Mrr, Mrc, Mcc) and status its catalogue row, aper_status and rho_auto its aperture row,
    place = (pr, pc) its stamp's top-left corner in the field, T (F, F, nb) the completed mean field, D the observed field
    or None.  Returns a dict of the six outputs and of the absolute sums ap_model_abs, ap_data_abs (K, nb), auto_model_abs,
    auto_data_abs (nb,)."""
    par = params() if par is None else par
    T = np.asarray(T, dtype=np.float64)
    D = None if D is None else np.asarray(D, dtype=np.float64)
    F, nb = T.shape[0], T.shape[2]
    R = [np.float64(v) for v in par["radii"]]
    K, s = len(R), int(par["subsample"])
    nan = np.float64(np.nan)
    out = dict(ap_model_sum=np.full((K, nb), nan), ap_data_sum=np.full((K, nb), nan), ap_field_area=np.full(K, nan),
               auto_model_sum=np.full(nb, nan), auto_data_sum=np.full(nb, nan), auto_field_area=nan,
               ap_model_abs=np.full((K, nb), nan), ap_data_abs=np.full((K, nb), nan), auto_model_abs=np.full(nb, nan),
               auto_data_abs=np.full(nb, nan))
    r0, c0, Mrr, Mrc, Mcc = (np.float64(v) for v in shape)
    with np.errstate(all="ignore"):
        det = Mrr * Mcc - Mrc * Mrc
        if aper_status == INELIGIBLE or status not in (0, 2) or not np.all(np.isfinite([r0, c0, Mrr, Mrc, Mcc])) or \
                not (np.isfinite(det) and det > 1e-6):
            return out
        circle = (np.float64(1.0), np.float64(0.0), np.float64(1.0))
        for k in range(K):
            cnt, _ = counts(cs, r0, c0, circle, R[k], s, shortcut)
            (out["ap_model_sum"][k], out["ap_data_sum"][k], out["ap_field_area"][k], out["ap_model_abs"][k],
             out["ap_data_abs"][k]) = _region(T, D, cnt, place, F, s)
        if aper_status != OK:
            return out
        form = (Mcc / det, (-2.0 * Mrc) / det, Mrr / det)
        cnt, _ = counts(cs, r0, c0, form, np.float64(rho_auto), s, shortcut)
        (out["auto_model_sum"], out["auto_data_sum"], out["auto_field_area"], out["auto_model_abs"],
         out["auto_data_abs"]) = _region(T, D, cnt, place, F, s)
    return out


def aperture_fields(shape, status, aper_status, kron, places, field_ptr, model_fields, data_fields, cs, par=None,
                    shortcut=False):
    """shape (N, 5), status (N,), aper_status (N,), kron (N, 3), places (N, 2), field_ptr (M + 1,), model_fields / data_fields
    (M, F, F, nb) (data_fields may be None) -> the list of the rows' dicts"""
    rows = []
    for m in range(len(field_ptr) - 1):
        for i in range(int(field_ptr[m]), int(field_ptr[m + 1])):
            rows.append(field_row(shape[i], int(status[i]), int(aper_status[i]), kron[i][1], places[i], model_fields[m],
                                  None if data_fields is None else data_fields[m], cs, par, shortcut))
    return rows


def stack(rows, key):
    return np.stack([np.asarray(r[key]) for r in rows]) if rows else np.zeros((0,))


def composite(stamps, places, F):
    """the mean field of one field: the float64 sum of its widened stamps at their placements in object order, off-field parts
    dropped"""
    stamps = np.asarray(stamps)
    cs, nb = stamps.shape[1], stamps.shape[3]
    T = np.zeros((F, F, nb), np.float64)
    for P, (pr, pc) in zip(stamps, places):
        pr, pc = int(pr), int(pc)
        r_lo, r_hi, c_lo, c_hi = max(0, -pr), min(cs, F - pr), max(0, -pc), min(cs, F - pc)
        if r_hi > r_lo and c_hi > c_lo:
            T[pr + r_lo:pr + r_hi, pc + c_lo:pc + c_hi] += P[r_lo:r_hi, c_lo:c_hi].astype(np.float64)
    return T
