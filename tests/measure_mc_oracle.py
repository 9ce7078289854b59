"""numpy float64 restatement of the Monte-Carlo catalogue: every sample stamp of every galaxy measured
with tests/measure_oracle.py, the measured rows folded per galaxy with Welford's recurrence in ascending sample order.  The
fold performs the scalar operations of the specification one by one, in its order, on numpy float64 scalars: given the same
per-sample rows it has the bits of the kernel.  It is the reference of tests/test_measure_mc_host.py and
tests/test_gpu_measure_mc.py."""
import numpy as np

from tests import measure_oracle as mo

SHAPE_NAMES = ("row", "col", "Mrr", "Mrc", "Mcc", "sigma", "e1", "e2")


def shape_row(moments, status):
    """(the 8 shape quantities of one sample, accepted?) from its {r0, c0, Mrr, Mrc, Mcc} and status"""
    r0, c0, Mrr, Mrc, Mcc = (np.float64(v) for v in moments)
    with np.errstate(all="ignore"):
        tr = Mcc + Mrr
        det = Mrr * Mcc - Mrc * Mrc
        if not (int(status) == 0 and det > 0.0 and tr > 0.0):
            return None, False
        sigma = np.sqrt(np.sqrt(det))
        e1 = (Mcc - Mrr) / tr
        e2 = np.float64(2.0) * Mrc / tr
    return np.array([r0, c0, Mrr, Mrc, Mcc, sigma, e1, e2], dtype=np.float64), True


def fold(sample_flux, sample_shape, sample_status):
    """Per-sample rows (N, S, nb), (N, S, 5), (N, S) -> dict(flux_mc_mean, flux_mc_std (N, nb), shape_mc_mean, shape_mc_std
    (N, 8), n_ok (N,)): Welford from (n, mean, M2) = 0 over q = 0 .. S - 1, std = sqrt(M2 / n); fluxes over all samples, the
    shape quantities over the accepted ones (n_ok = 0: NaN)."""
    sample_flux = np.asarray(sample_flux, dtype=np.float64)
    N, S, nb = sample_flux.shape
    out = dict(flux_mc_mean=np.zeros((N, nb)), flux_mc_std=np.zeros((N, nb)), shape_mc_mean=np.zeros((N, 8)),
               shape_mc_std=np.zeros((N, 8)), n_ok=np.zeros(N, np.int32))
    zero = np.float64(0.0)
    with np.errstate(all="ignore"):
        for i in range(N):
            for b in range(nb):
                mean, m2 = zero, zero
                for q in range(S):
                    x = sample_flux[i, q, b]
                    d = x - mean
                    mean = mean + d / np.float64(q + 1)
                    m2 = m2 + d * (x - mean)
                out["flux_mc_mean"][i, b] = mean
                out["flux_mc_std"][i, b] = np.sqrt(m2 / np.float64(S))
            mean, m2, n = [zero] * 8, [zero] * 8, 0
            for q in range(S):
                row, ok = shape_row(sample_shape[i, q], sample_status[i, q])
                if not ok:
                    continue
                n += 1
                for k in range(8):
                    d = row[k] - mean[k]
                    mean[k] = mean[k] + d / np.float64(n)
                    m2[k] = m2[k] + d * (row[k] - mean[k])
            out["n_ok"][i] = n
            for k in range(8):
                out["shape_mc_mean"][i, k] = mean[k] if n else np.nan
                out["shape_mc_std"][i, k] = np.sqrt(m2[k] / np.float64(n)) if n else np.nan
    return out


def measure_mc(samples, band=2, sigma0=3.0, tol=1e-10, max_iter=200):
    """samples (S, N, cs, cs, nb) -> fold()'s dictionary plus the per-sample rows sample_flux (N, S, nb), sample_shape
    (N, S, 5), sample_status (N, S) and sample_iters (N, S)."""
    samples = np.asarray(samples)
    S, N = samples.shape[:2]
    per = [mo.measure(samples[q], None, band, sigma0, tol, max_iter) for q in range(S)]
    rows = dict(sample_flux=np.stack([p["flux"] for p in per], axis=1) if S else np.zeros((N, 0, samples.shape[4])),
                sample_shape=np.stack([p["shape"] for p in per], axis=1),
                sample_status=np.stack([p["status"] for p in per], axis=1).astype(np.int32),
                sample_iters=np.stack([p["iters"] for p in per], axis=1).astype(np.int32))
    out = fold(rows["sample_flux"], rows["sample_shape"], rows["sample_status"])
    out.update(rows)
    return out


def direct(sample_flux, sample_shape, sample_status):
    """The same statistics taken directly: np.mean / np.std over the accepted samples (the check of fold())."""
    sample_flux = np.asarray(sample_flux, dtype=np.float64)
    N = sample_flux.shape[0]
    out = dict(flux_mc_mean=sample_flux.mean(axis=1), flux_mc_std=sample_flux.std(axis=1),
               shape_mc_mean=np.full((N, 8), np.nan), shape_mc_std=np.full((N, 8), np.nan), n_ok=np.zeros(N, np.int32))
    for i in range(N):
        rows = [r for r, ok in (shape_row(m, s) for m, s in zip(sample_shape[i], sample_status[i])) if ok]
        out["n_ok"][i] = len(rows)
        if rows:
            out["shape_mc_mean"][i] = np.mean(rows, axis=0)
            out["shape_mc_std"][i] = np.std(rows, axis=0)
    return out


def jittered_gaussians(cs, nb, S, seed, M=(6.0, 1.0, 8.0), amp=2.0):
    """(S, cs, cs, nb) float32: one galaxy's samples - an elliptical Gaussian whose offset, axis ratio, size and amplitude jitter
    from sample to sample, the same plane rescaled in every band"""
    rng = np.random.default_rng(seed)
    out = np.zeros((S, cs, cs, nb), np.float32)
    for q in range(S):
        f = 1.0 + rng.uniform(-0.15, 0.15)
        Mq = (M[0] * f, M[1] * (1.0 + rng.uniform(-0.3, 0.3)), M[2] / f * (1.0 + rng.uniform(-0.1, 0.1)))
        g = mo.gaussian_stamp(cs, Mq, rng.uniform(-0.6, 0.6, size=2), amp * (1.0 + rng.uniform(-0.1, 0.1)))
        out[q] = g[:, :, None] * (0.5 + 0.25 * np.arange(nb))
    return out


def spike_stamp(cs, nb):
    s = np.zeros((cs, cs, nb), np.float32)
    s[cs // 2, cs // 2] = 5.0
    return s
