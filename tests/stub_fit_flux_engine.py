"""Stand-ins for the engine and its context in the CPU tests of the simultaneous flux fit (tests/test_fit_flux_host.py), in the
manner of tests/stub_aperture_fields_engine.py: no GPU, no HIP.  The context answers scene_fit_flux with the numpy restatement
of tests/fit_flux_oracle.py; the engine records its calls and returns rows that encode the global stamp number."""
import numpy as np

from tests import fit_flux_oracle as fo
from tests import stub_measure_engine as sm

CS, NB = sm.CS, sm.NB
KEYS = ("fit_scale", "fit_var", "fit_gram", "fit_proj", "fit_status")


class OracleContext(sm.OracleContext):
    def scene_fit_flux(self, stamps, places, data_fields, field_ptr=None, min_pivot=1e-8, scratch_bytes=256 << 20):
        stamps = np.asarray(stamps, dtype=np.float32)
        data = np.asarray(data_fields, dtype=np.float64)
        n = len(stamps)
        self.calls.append(dict(fit_flux=n, fields=data.shape[0], min_pivot=min_pivot,
                               field_ptr=None if field_ptr is None else list(field_ptr)))
        out, _ = fo.fit_flux(stamps, places, [0, n] if field_ptr is None else field_ptr, data, min_pivot)
        return {k: out[k] for k in KEYS}


def stub_fit_flux(n, nb):
    """Rows that encode their number: galaxy i has fit_scale[b] = 1 + 0.01 i + 0.001 b, fit_gram = 50 + i + b, fit_var = 1.25 /
    fit_gram (independence sqrt(0.8)), fit_proj = 1.5 fit_gram; row 1 is dropped in band 0 (status 5: scale 1, var NaN), every
    fifth row from 4 on is ineligible in the last band (status 4: scale and var NaN, fit_gram 0)"""
    i, b = np.arange(n, dtype=np.float64)[:, None], np.arange(nb, dtype=np.float64)[None, :]
    out = dict(fit_scale=1.0 + 0.01 * i + 0.001 * b, fit_gram=50.0 + i + b, fit_status=np.zeros((n, nb), np.int32))
    out["fit_var"] = 1.25 / out["fit_gram"]
    out["fit_proj"] = 1.5 * out["fit_gram"]
    if n > 1:
        out["fit_status"][1, 0], out["fit_scale"][1, 0], out["fit_var"][1, 0] = 5, 1.0, np.nan
    bad = np.arange(n) % 5 == 4
    out["fit_status"][bad, -1] = 4
    out["fit_scale"][bad, -1] = out["fit_var"][bad, -1] = np.nan
    out["fit_gram"][bad, -1] = out["fit_proj"][bad, -1] = 0.0
    return out


class RecordingEngine(sm.RecordingEngine):
    def infer_fields_measure_fit(self, fields, starts, field_ptr, places, seed=0, band=2, sigma0=3.0, tol=1e-10, max_iter=200,
                                 min_pivot=1e-8, scratch_bytes=256 << 20, return_fields=True, residual=True, mse_center=True):
        out = self.infer_fields_measure(fields, starts, field_ptr, places=places if return_fields else None, seed=seed,
                                        return_fields=return_fields)
        self.calls.pop(-1)
        self.calls.append(("infer_fields_measure_fit", seed, return_fields, None if places is None else np.array(places),
                           min_pivot))
        out.update(stub_fit_flux(len(starts), fields.shape[3]))
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
