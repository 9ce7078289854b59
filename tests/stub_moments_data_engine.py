"""Stand-ins for the engine and its context in the CPU tests of the moments on the observed field
(tests/test_moments_data_host.py), in the manner of tests/stub_fit_flux_groups_engine.py: no GPU, no HIP.  The context answers
scene_moments_fields with the numpy restatement of tests/moments_fields_oracle.py; the engine records its calls and returns rows
that encode the global stamp number."""
import numpy as np

from tests import moments_fields_oracle as mf
from tests import stub_fit_flux_groups_engine as sg

CS, NB = sg.CS, sg.NB
MKEYS = ("flux_data", "npix_data", "shape_data", "iters_data", "status_data")


class OracleContext(sg.OracleContext):
    def scene_moments_fields(self, stamps, places, model_fields, data_fields, weight_fields=None, field_ptr=None, band=2,
                             sigma0=3.0, tol=1e-10, max_iter=200):
        stamps = np.asarray(stamps, dtype=np.float32)
        model, data = np.asarray(model_fields, dtype=np.float64), np.asarray(data_fields, dtype=np.float64)
        n = len(stamps)
        self.calls.append(dict(moments_fields=n, fields=model.shape[0], band=band, sigma0=sigma0, tol=tol, max_iter=max_iter,
                               weights=None if weight_fields is None else np.shape(weight_fields),
                               field_ptr=None if field_ptr is None else list(field_ptr)))
        weights = None if weight_fields is None else np.asarray(weight_fields, dtype=np.float64)
        if weights is not None and weights.ndim == 3:                  # (one field, as Context.scene_moments_fields takes it)
            weights = weights[None]
        out = mf.moments_fields(stamps, places, [0, n] if field_ptr is None else field_ptr, model, data, weights, band, sigma0,
                                tol, max_iter)
        return {k: out[k] for k in MKEYS}


def stub_moments_data(n, nb):
    """Rows that encode their number: flux_data = 10 i + b + 0.5, npix_data = 900 - i - b, shape_data = {15 + 0.01 i, 15 - 0.01 i,
    4 + 0.1 i, 0.5, 3}, iters_data = 20 + i, status_data = 3 for every fourth row from row 3 on, else 0"""
    i, b = np.arange(n)[:, None], np.arange(nb)[None, :]
    k = np.arange(n)
    return dict(flux_data=10.0 * i + b + 0.5, npix_data=(900 - i - b).astype(np.int32),
                shape_data=np.stack([15 + 0.01 * k, 15 - 0.01 * k, 4 + 0.1 * k, np.full(n, 0.5), np.full(n, 3.0)], axis=1),
                iters_data=(20 + k).astype(np.int32), status_data=np.where(k % 4 == 3, 3, 0).astype(np.int32))


class RecordingEngine(sg.RecordingEngine):
    def infer_fields_measure_moments_data(self, fields, starts, field_ptr, places, weight_fields=None, seed=0, band=2, sigma0=3.0,
                                          tol=1e-10, max_iter=200, return_fields=True, residual=True, mse_center=True):
        out = self.infer_fields_measure(fields, starts, field_ptr, places=places if return_fields else None, seed=seed,
                                        return_fields=return_fields)
        self.calls.pop(-1)
        self.calls.append(("infer_fields_measure_moments_data", seed, return_fields, None if places is None else np.array(places),
                           None if weight_fields is None else np.asarray(weight_fields), band))
        out.update(stub_moments_data(len(starts), fields.shape[3]))
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
