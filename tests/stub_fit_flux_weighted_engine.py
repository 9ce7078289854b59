"""Stand-ins for the engine and its context in the CPU tests of the weighted flux fit (tests/test_fit_flux_weighted_host.py), in
the manner of tests/stub_fit_flux_engine.py: no GPU, no HIP.  The context answers scene_fit_flux(weight_fields=...) with the
numpy restatement of tests/fit_flux_weighted_oracle.py; the engine records its calls and returns rows that encode the global
stamp number."""
import numpy as np

from tests import fit_flux_weighted_oracle as fw
from tests import stub_fit_flux_engine as sf

CS, NB = sf.CS, sf.NB
KEYS = sf.KEYS
WKEYS = KEYS + ("fit_chi2", "fit_npix")


class OracleContext(sf.OracleContext):
    def scene_fit_flux(self, stamps, places, data_fields, field_ptr=None, min_pivot=1e-8, scratch_bytes=256 << 20,
                       weight_fields=None):
        if weight_fields is None:
            return super().scene_fit_flux(stamps, places, data_fields, field_ptr=field_ptr, min_pivot=min_pivot)
        stamps = np.asarray(stamps, dtype=np.float32)
        data, weights = np.asarray(data_fields, dtype=np.float64), np.asarray(weight_fields, dtype=np.float64)
        n = len(stamps)
        self.calls.append(dict(fit_flux_weighted=n, fields=data.shape[0], min_pivot=min_pivot, weights=weights.shape,
                               field_ptr=None if field_ptr is None else list(field_ptr)))
        out, _ = fw.fit_flux(stamps, places, [0, n] if field_ptr is None else field_ptr, data, weights, min_pivot)
        return {k: out[k] for k in WKEYS}


def stub_fit_flux_weighted(n, nb):
    """stub_fit_flux's rows, and: fit_npix = 100 + 3 i + b, fit_chi2 = fit_npix - 1 + 0.25 b; an ineligible row (status 4) has
    fit_npix 0 and fit_chi2 NaN"""
    out = sf.stub_fit_flux(n, nb)
    i, b = np.arange(n)[:, None], np.arange(nb)[None, :]
    out["fit_npix"] = (100 + 3 * i + b).astype(np.int32)
    out["fit_chi2"] = out["fit_npix"] - 1.0 + 0.25 * b
    bad = out["fit_status"] == 4
    out["fit_npix"][bad] = 0
    out["fit_chi2"][bad] = np.nan
    return out


class RecordingEngine(sf.RecordingEngine):
    def infer_fields_measure_fit_weighted(self, fields, starts, field_ptr, places, weight_fields, seed=0, band=2, sigma0=3.0,
                                          tol=1e-10, max_iter=200, min_pivot=1e-8, scratch_bytes=256 << 20, return_fields=True,
                                          residual=True, mse_center=True):
        out = self.infer_fields_measure(fields, starts, field_ptr, places=places if return_fields else None, seed=seed,
                                        return_fields=return_fields)
        self.calls.pop(-1)
        self.calls.append(("infer_fields_measure_fit_weighted", seed, return_fields, None if places is None else np.array(places),
                           np.asarray(weight_fields)))
        out.update(stub_fit_flux_weighted(len(starts), fields.shape[3]))
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
