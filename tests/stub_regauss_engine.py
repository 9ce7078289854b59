"""Stand-ins for the engine and its context in the CPU tests of the PSF correction (tests/test_regauss_host.py), in the manner
of tests/stub_measure_engine.py: no GPU, no HIP.  The context answers scene_measure and scene_regauss with the numpy
restatements; the engine records its calls and returns rows that encode the global stamp number."""
import numpy as np

from tests import regauss_oracle as ro
from tests import stub_measure_engine as sm

CS, NB = sm.CS, sm.NB


class OracleContext(sm.OracleContext):
    def scene_regauss(self, stamps, shape, status, psf, psf_index=None, band=2, psf_sigma0=2.0, tol=1e-10, max_iter=200):
        psf = np.asarray(psf, dtype=np.float64)
        psf = psf[None] if psf.ndim == 2 else psf
        index = np.zeros(len(stamps), np.int32) if psf_index is None else np.asarray(psf_index)
        self.calls.append(dict(regauss=len(stamps), K=len(psf), index=index.copy(), band=band, psf_sigma0=psf_sigma0))
        return ro.regauss(stamps, shape, status, index, psf, band, psf_sigma0, tol, max_iter)


def stub_regauss(n, K):
    """Rows that encode their number: stamp i has M' = (9 + i, 0.5, 12 + i), every fourth row unresolved; PSF k has
    M_P = (2 + k, 0.25, 3 + k)"""
    i = np.arange(n, dtype=np.float64)
    st = np.where(np.arange(n) % 4 == 3, 6, 0).astype(np.int32)
    rg = np.stack([29.0 + 0.125 * i, 29.0 - 0.25 * i, 9.0 + i, 0.5 * np.ones(n), 12.0 + i, 2.0 + 0.01 * i], axis=1).reshape(n, 6)
    rg[st == 6] = np.nan
    k = np.arange(K, dtype=np.float64)
    return dict(regauss=rg, regauss_iters=np.where(st == 0, 30 + np.arange(n), 0).astype(np.int32), regauss_status=st,
                psf_shape=np.stack([10.0 + 0 * k, 10.0 + 0 * k, 2.0 + k, 0.25 + 0 * k, 3.0 + k], axis=1).reshape(K, 5),
                psf_aux=np.stack([0.1 + 0 * k, 1.0 + 0 * k, 2.05 + 0.01 * k], axis=1).reshape(K, 3),
                psf_iters=np.full(K, 33, np.int32), psf_status=np.zeros(K, np.int32))


class RecordingEngine(sm.RecordingEngine):
    def infer_fields_measure_psf(self, fields, starts, field_ptr, psf, psf_index=None, places=None, seed=0, band=2, sigma0=3.0,
                                 tol=1e-10, max_iter=200, psf_sigma0=2.0, return_fields=True, residual=True, mse_center=True):
        out = self.infer_fields_measure(fields, starts, field_ptr, places=places, seed=seed, return_fields=return_fields)
        self.calls.pop(-1)
        self.calls.append(("infer_fields_measure_psf", seed, return_fields, None if places is None else np.array(places),
                           np.array(psf), None if psf_index is None else np.array(psf_index)))
        out.update(stub_regauss(len(starts), len(psf)))
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
