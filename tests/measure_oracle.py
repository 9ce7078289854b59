"""numpy float64 restatement of the catalogue measurement: per-band fluxes and their errors and the
adaptive moments of one band of a stamp.  Written from the specification, not from the kernel; it is the reference of
tests/test_measure_host.py and tests/test_gpu_measure.py, and tools/measure_bench.py times it as the host route."""
import numpy as np

CONVERGED, ITER_LIMIT, FAILED = 0, 2, 3


def adaptive_moments(I, sigma0=3.0, tol=1e-10, max_iter=200, history=None):
    """One band plane I (cs, cs) -> ((r0, c0, Mrr, Mrc, Mcc), iters, status).  history: a list that receives every
    iteration's max(step, dM), the quantity the stop test bounds (the step alone is rounding noise on a symmetric stamp,
    whose iteration moves only M)."""
    I = np.asarray(I, dtype=np.float64)
    cs = I.shape[0]
    assert I.shape == (cs, cs)
    r = np.arange(cs, dtype=np.float64)[:, None]
    c = np.arange(cs, dtype=np.float64)[None, :]
    ctr = (cs - 1) / 2.0
    r0 = c0 = ctr
    Mrr = Mcc = float(sigma0) ** 2
    Mrc = 0.0
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
            if history is not None:
                history.append(max(step, float(dM)))
            r0, c0 = r0 + 2.0 * mr, c0 + 2.0 * mc
            Mrr, Mrc, Mcc = Nrr, Nrc, Ncc
            # the centroid has left the stamp, or the trace is negative or not finite (a zero trace - a one-pixel spike -
            # goes on and ends at the next iteration's determinant test)
            if not abs(r0 - ctr) <= cs / 2.0 or not abs(c0 - ctr) <= cs / 2.0 or not (np.isfinite(tr) and tr >= 0.0):
                status = FAILED
                break
            if step < tol and dM < tol:
                status = CONVERGED
                break
    return np.array([r0, c0, Mrr, Mrc, Mcc], dtype=np.float64), it, status


def measure(mean, stddev=None, band=2, sigma0=3.0, tol=1e-10, max_iter=200, histories=None):
    """mean / stddev (N, cs, cs, nb) -> dict(flux (N, nb), flux_err (N, nb) or None, shape (N, 5), iters (N,), status (N,))."""
    P = np.asarray(mean).astype(np.float64)
    n, cs, _, nb = P.shape
    out = {"flux": P.reshape(n, cs * cs, nb).sum(axis=1), "flux_err": None, "shape": np.zeros((n, 5)),
           "iters": np.zeros(n, np.int32), "status": np.zeros(n, np.int32)}
    if stddev is not None:
        S = np.asarray(stddev).astype(np.float64)
        out["flux_err"] = np.sqrt((S * S).reshape(n, cs * cs, nb).sum(axis=1))
    for i in range(n):
        h = [] if histories is not None else None
        out["shape"][i], out["iters"][i], out["status"][i] = adaptive_moments(P[i, :, :, band], sigma0, tol, max_iter, h)
        if histories is not None:
            histories.append(h)
    return out


def gaussian_stamp(cs, M, offset, amp=1.0):
    """Noise-free elliptical Gaussian with moment matrix M = (Mrr, Mrc, Mcc) centred at (cs - 1) / 2 + offset."""
    Mrr, Mrc, Mcc = M
    det = Mrr * Mcc - Mrc * Mrc
    r = np.arange(cs, dtype=np.float64)[:, None] - ((cs - 1) / 2.0 + offset[0])
    c = np.arange(cs, dtype=np.float64)[None, :] - ((cs - 1) / 2.0 + offset[1])
    return amp * np.exp(-0.5 * (Mcc * r * r - 2.0 * Mrc * r * c + Mrr * c * c) / det)
