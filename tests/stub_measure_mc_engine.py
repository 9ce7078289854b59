"""Stand-ins for the engine and its context in the CPU tests of the Monte-Carlo catalogue (tests/test_measure_mc_host.py), in
the manner of tests/stub_measure_engine.py: no GPU, no HIP.  The context answers scene_measure_mc with the numpy oracle; the
engine records its calls and returns catalogues that encode the global stamp number."""
import numpy as np

from tests import measure_mc_oracle as mmo
from tests import stub_measure_engine as base

CS, NB = base.CS, base.NB


class OracleMcContext(base.OracleContext):
    """Context.scene_measure_mc answered by tests/measure_mc_oracle.py"""

    def scene_measure_mc(self, samples, band=2, sigma0=3.0, tol=1e-10, max_iter=200, keep_samples=False):
        self.calls.append(dict(S=samples.shape[0], n=samples.shape[1], band=band, sigma0=sigma0, tol=tol, max_iter=max_iter,
                               dtype=samples.dtype, keep_samples=keep_samples))
        out = mmo.measure_mc(samples, band, sigma0, tol, max_iter)
        del out["sample_iters"]
        if not keep_samples:
            for k in ("sample_flux", "sample_shape", "sample_status"):
                del out[k]
        return out


def stub_mc_catalogue(n, nb=NB):
    """A Monte-Carlo catalogue whose row i encodes i; every fourth galaxy had no accepted sample"""
    i = np.arange(n, dtype=np.float64)
    none = np.arange(n) % 4 == 3
    mean = 100.0 * i[:, None] + np.arange(8)[None, :]
    std = 0.01 * (i[:, None] + 1) + 0.001 * np.arange(8)[None, :]
    return dict(flux_mc_mean=1000.0 + i[:, None] + np.arange(nb)[None, :], flux_mc_std=0.5 * (i[:, None] + 1) * np.ones((1, nb)),
                shape_mc_mean=np.where(none[:, None], np.nan, mean), shape_mc_std=np.where(none[:, None], np.nan, std),
                n_ok=np.where(none, 0, 3).astype(np.int32))


class RecordingMcEngine(base.RecordingEngine):
    def infer_fields_measure_mc(self, fields, starts, field_ptr, places=None, seed=0, mc_seed=0, nsamples=100, band=2,
                                sigma0=3.0, tol=1e-10, max_iter=200, return_fields=True, residual=True, mse_center=True,
                                keep_samples=False):
        out = self.infer_fields_measure(fields, starts, field_ptr, places=places, seed=seed, return_fields=return_fields)
        self.calls.pop(-1)
        self.calls.append(("infer_fields_measure_mc", seed, mc_seed, nsamples, return_fields,
                           None if places is None else np.array(places)))
        out.update(stub_mc_catalogue(len(starts), fields.shape[3]))
        return out


class Core(base.Core):
    def __init__(self):
        self.engine, self.ctx, self.seed_counter = RecordingMcEngine(), OracleMcContext(), 7


class Net:
    def __init__(self):
        self._core = Core()
