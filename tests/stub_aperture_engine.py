"""Stand-ins for the engine and its context in the CPU tests of the aperture photometry (tests/test_aperture_host.py), in the
manner of tests/stub_measure_engine.py: no GPU, no HIP.  The context answers scene_measure and scene_aperture with the numpy
restatements; the engine records its calls and returns rows that encode the global stamp number."""
import numpy as np

from tests import aperture_oracle as ao
from tests import stub_measure_engine as sm

CS, NB = sm.CS, sm.NB


class OracleContext(sm.OracleContext):
    def scene_aperture(self, mean, shape, status, stddev=None, radii=(3.0, 5.0, 8.0), fractions=(0.2, 0.5, 0.8), band=2,
                       subsample=5, kron_factor=2.5, kron_min=3.5, kron_limit=6.0, bisect_iters=32):
        self.calls.append(dict(aperture=len(mean), radii=tuple(radii), fractions=tuple(fractions), band=band,
                               with_stddev=stddev is not None))
        par = ao.params(radii=tuple(radii), fractions=tuple(fractions), subsample=subsample, kron_factor=kron_factor,
                        kron_min=kron_min, kron_limit=kron_limit, bisect_iters=bisect_iters)
        rows = ao.aperture(mean, stddev, shape, status, band, par, shortcut=True)
        n, nb, K, J = len(mean), mean.shape[3], len(par["radii"]), len(par["fractions"])
        stack = lambda key, tail: np.array([r[key] for r in rows], dtype=np.float64).reshape((n,) + tail)
        out = dict(ap_flux=stack("ap_flux", (K, nb)), ap_area=stack("ap_area", (K,)), flux_auto=stack("flux_auto", (nb,)),
                   kron=stack("kron", (3,)), flux_rho=stack("flux_rho", (J,)),
                   aper_flags=np.array([r["flags"] for r in rows], np.int32).reshape(n),
                   aper_status=np.array([r["status"] for r in rows], np.int32).reshape(n))
        if stddev is not None:
            out.update(ap_flux_err=stack("ap_flux_err", (K, nb)), flux_auto_err=stack("flux_auto_err", (nb,)))
        return out


def stub_aperture(n, nb, K, J):
    """Rows that encode their number: stamp i has ap_flux[k][b] = 100 i + 10 k + b, rho_auto = 3.5 + i, flux_rho[j] = (j + 1) /
    (J + 1) of it; row 1 has no Kron radius (status 7), every fifth row from 4 on is ineligible (status 4)"""
    i = np.arange(n, dtype=np.float64)
    st = np.where(np.arange(n) % 5 == 4, 4, np.where(np.arange(n) == 1, 7, 0)).astype(np.int32)
    apf = 100.0 * i[:, None, None] + 10.0 * np.arange(K)[None, :, None] + np.arange(nb)[None, None, :]
    area = 3.0 + i[:, None] + np.arange(K)[None, :]
    fauto = 7.0 + i[:, None] + 0.5 * np.arange(nb)[None, :]
    kron = np.stack([1.25 + 0.01 * i, 3.5 + i, 40.0 + i], axis=1).reshape(n, 3)
    frho = (3.5 + i[:, None]) * (np.arange(J)[None, :] + 1.0) / (J + 1.0)
    out = dict(ap_flux=apf, ap_flux_err=0.01 * apf, ap_area=area, flux_auto=fauto, flux_auto_err=0.1 * fauto, kron=kron,
               flux_rho=frho, aper_flags=np.where(st == 0, 1 << 10, 0).astype(np.int32), aper_status=st)
    for k in ("flux_auto", "flux_auto_err", "kron", "flux_rho"):
        out[k][st != 0] = np.nan
    for k in ("ap_flux", "ap_flux_err", "ap_area"):
        out[k][st == 4] = np.nan
    return out


class RecordingEngine(sm.RecordingEngine):
    def infer_fields_measure_aper(self, fields, starts, field_ptr, places=None, seed=0, band=2, sigma0=3.0, tol=1e-10,
                                  max_iter=200, radii=(3.0, 5.0, 8.0), fractions=(0.2, 0.5, 0.8), subsample=5, kron_factor=2.5,
                                  kron_min=3.5, kron_limit=6.0, bisect_iters=32, return_fields=True, residual=True,
                                  mse_center=True):
        out = self.infer_fields_measure(fields, starts, field_ptr, places=places, seed=seed, return_fields=return_fields)
        self.calls.pop(-1)
        self.calls.append(("infer_fields_measure_aper", seed, return_fields, None if places is None else np.array(places),
                           tuple(radii), tuple(fractions)))
        out.update(stub_aperture(len(starts), fields.shape[3], len(radii), len(fractions)))
        return out


class Core:
    def __init__(self):
        self.engine, self.ctx, self.seed_counter = RecordingEngine(), OracleContext(), 7

    def next_seed(self):
        self.seed_counter += 1
        return self.seed_counter


class Net:
    def __init__(self):
        self._core = Core()
