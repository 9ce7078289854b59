"""Stand-ins for the engine and its context in the CPU tests of the non-negative flux fit (tests/test_fit_flux_nonneg_host.py),
in the manner of tests/stub_fit_flux_sky_engine.py: no GPU, no HIP.  The context answers scene_fit_flux_nonneg with the numpy
restatement of tests/fit_flux_nonneg_oracle.py; the engine records its calls and returns rows that encode the global stamp
number and per-field arrays that encode the field."""
import numpy as np

from tests import fit_flux_nonneg_oracle as fn
from tests import stub_fit_flux_sky_engine as ss

CS, NB = ss.CS, ss.NB
KEYS, WKEYS, SKY_KEYS = ss.KEYS, ss.WKEYS, ss.SKY_KEYS
NONNEG_KEYS = ("fit_scale_free", "fit_clamped", "fit_dual")
NONNEG_FIELD_KEYS = ("nonneg_iters", "nonneg_status")


class OracleContext(ss.OracleContext):
    def scene_fit_flux_nonneg(self, stamps, places, data_fields, field_ptr=None, sky_order=None, weight_fields=None,
                              min_pivot=1e-8, max_iter=100, scratch_bytes=256 << 20):
        stamps = np.asarray(stamps, dtype=np.float32)
        data = np.asarray(data_fields, dtype=np.float64)
        n = len(stamps)
        self.calls.append(dict(fit_flux_nonneg=n, fields=data.shape[0], sky_order=sky_order, min_pivot=min_pivot, max_iter=max_iter,
                               weights=None if weight_fields is None else np.shape(weight_fields),
                               field_ptr=None if field_ptr is None else list(field_ptr)))
        out, _ = fn.fit_flux_nonneg(stamps, places, [0, n] if field_ptr is None else field_ptr, data, sky_order, weight_fields,
                                    min_pivot, max_iter)
        keys = (KEYS if weight_fields is None else WKEYS) + (() if sky_order is None else SKY_KEYS)
        return {k: out[k] for k in keys + NONNEG_KEYS + NONNEG_FIELD_KEYS}


def stub_nonneg(rows, M, nb):
    """`rows` (the stub rows of the fit without the constraint, changed in place) as a non-negative fit would return them, and
    its own arrays: every third galaxy from 2 on is clamped in band 1 where its status is 0 - fit_scale +0.0, fit_var NaN,
    fit_scale_free = -(0.1 + 0.01 i), fit_dual = 2 + i -; elsewhere fit_scale_free = fit_scale and fit_dual = +0.0, NaN where the
    status is not 0; nonneg_iters[m, b] = 1 + (m + b) % 3, nonneg_status 0 but 1 for the last band of field 0"""
    n = rows["fit_scale"].shape[0]
    i = np.arange(n)[:, None]
    z = np.zeros((n, nb), bool)
    if nb > 1:
        z[2::3, 1] = True
    z &= rows["fit_status"] == 0
    free = np.where(z, -(0.1 + 0.01 * i), rows["fit_scale"])
    rows["fit_scale"] = np.where(z, 0.0, rows["fit_scale"])
    rows["fit_var"] = np.where(z, np.nan, rows["fit_var"])
    dual = np.where(rows["fit_status"] == 0, np.where(z, 2.0 + i, 0.0), np.nan)
    m, b = np.arange(M)[:, None], np.arange(nb)[None, :]
    status = np.zeros((M, nb), np.int32)
    if M:
        status[0, -1] = 1
    return dict(fit_scale_free=free, fit_clamped=z.astype(np.int32), fit_dual=dual,
                nonneg_iters=(1 + (m + b) % 3).astype(np.int32), nonneg_status=status)


class RecordingEngine(ss.RecordingEngine):
    def infer_fields_measure_fit_nonneg(self, fields, starts, field_ptr, places, sky_order=None, weight_fields=None, seed=0,
                                        band=2, sigma0=3.0, tol=1e-10, max_iter=200, min_pivot=1e-8, fit_max_iter=100,
                                        scratch_bytes=256 << 20, return_fields=True, residual=True, mse_center=True):
        out = self.infer_fields_measure(fields, starts, field_ptr, places=places if return_fields else None, seed=seed,
                                        return_fields=return_fields)
        self.calls.pop(-1)
        self.calls.append(("infer_fields_measure_fit_nonneg", seed, return_fields, None if places is None else np.array(places),
                           sky_order, None if weight_fields is None else np.asarray(weight_fields), fit_max_iter))
        f = ss.sw.stub_fit_flux_weighted(len(starts), fields.shape[3])
        rows = {k: f[k] for k in (KEYS if weight_fields is None else WKEYS)}
        nn = stub_nonneg(rows, fields.shape[0], fields.shape[3])
        out.update(rows)
        if sky_order is not None:
            out.update(ss.stub_sky(fields.shape[0], fields.shape[3], 1 if sky_order == 0 else 3, fields.shape[1]))
        out.update(nn)
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
