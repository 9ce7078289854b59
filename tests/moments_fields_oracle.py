"""numpy float64 restatement of the adaptive moments on the observed field with the neighbours subtracted (DESIGN.md section
7x): the child image C = (D - T) + P of every galaxy exactly as the section defines it - two roundings in that order where the
stamp pixel counts, P elsewhere -, its per-band sums and counting pixels, and tests/measure_oracle.adaptive_moments on its band
plane.  Written from the specification, not from the kernel; it is the reference of tests/test_moments_data_host.py and
tests/test_gpu_moments_data.py."""
import numpy as np

from tests import measure_oracle as mo


def counts(w):
    """the rule of section 7s: a weight counts iff it lies in (0, inf)"""
    w = np.asarray(w, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (w > 0.0) & (w < np.inf)


def child_images(stamps, places, field_ptr, model_fields, data_fields, weight_fields=None):
    """(C (N, cs, cs, nb) float64, on (N, cs, cs, nb) bool): the child images and the counting pixels"""
    P = np.asarray(stamps, dtype=np.float32).astype(np.float64)
    n, cs, _, nb = P.shape
    T, D = np.asarray(model_fields, dtype=np.float64), np.asarray(data_fields, dtype=np.float64)
    F = T.shape[1]
    places = np.asarray(places, dtype=np.int64).reshape(n, 2)
    fp = np.asarray(field_ptr, dtype=np.int64)
    C, on = P.copy(), np.zeros(P.shape, dtype=bool)
    for m in range(len(fp) - 1):
        for i in range(int(fp[m]), int(fp[m + 1])):
            pr, pc = int(places[i, 0]), int(places[i, 1])
            ra, rz, ca, cz = max(pr, 0), min(pr + cs, F), max(pc, 0), min(pc + cs, F)
            if rz <= ra or cz <= ca:
                continue
            win = (slice(ra - pr, rz - pr), slice(ca - pc, cz - pc))
            sel = np.ones((rz - ra, cz - ca, nb), dtype=bool) if weight_fields is None else counts(weight_fields[m][ra:rz, ca:cz])
            with np.errstate(all="ignore"):
                resid = D[m, ra:rz, ca:cz] - T[m, ra:rz, ca:cz]              # the first rounding
                child = resid + P[i][win]                                    # the second
            C[i][win] = np.where(sel, child, P[i][win])
            on[i][win] = sel
    return C, on


def moments_fields(stamps, places, field_ptr, model_fields, data_fields, weight_fields=None, band=2, sigma0=3.0, tol=1e-10,
                   max_iter=200, histories=None):
    """dict(flux_data (N, nb), flux_abs (N, nb): the sum of |C|, the yardstick of the flux bound, npix_data (N, nb) int32,
    shape_data (N, 5), iters_data (N,), status_data (N,)); histories: a list that receives every row's list of max(step, dM)"""
    C, on = child_images(stamps, places, field_ptr, model_fields, data_fields, weight_fields)
    n, cs, _, nb = C.shape
    with np.errstate(all="ignore"):
        out = {"flux_data": C.reshape(n, cs * cs, nb).sum(axis=1), "flux_abs": np.abs(C).reshape(n, cs * cs, nb).sum(axis=1),
               "npix_data": on.reshape(n, cs * cs, nb).sum(axis=1).astype(np.int32), "shape_data": np.zeros((n, 5)),
               "iters_data": np.zeros(n, np.int32), "status_data": np.zeros(n, np.int32)}
    for i in range(n):
        h = [] if histories is not None else None
        out["shape_data"][i], out["iters_data"][i], out["status_data"][i] = mo.adaptive_moments(C[i, :, :, band], sigma0, tol,
                                                                                               max_iter, h)
        if histories is not None:
            histories.append(h)
    return out


def late_contraction(history, last=5):
    """rho of a converged iteration from its history of max(step, dM): the largest ratio of successive entries over the last
    `last` iterations (inf where there are too few entries or one of them is 0)"""
    h = np.asarray(history, dtype=np.float64)[-(last + 1):]
    if len(h) < 2 or not (h[:-1] > 0).all():
        return np.inf
    return float((h[1:] / h[:-1]).max())
