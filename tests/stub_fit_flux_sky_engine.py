"""Stand-ins for the engine and its context in the CPU tests of the flux fit with sky (tests/test_fit_flux_sky_host.py), in the
manner of tests/stub_fit_flux_weighted_engine.py: no GPU, no HIP.  The context answers scene_fit_flux_sky with the numpy
restatement of tests/fit_flux_sky_oracle.py; the engine records its calls and returns rows that encode the global stamp number
and per-field arrays that encode the field."""
import numpy as np

from tests import fit_flux_sky_oracle as fs
from tests import stub_fit_flux_weighted_engine as sw

CS, NB = sw.CS, sw.NB
KEYS, WKEYS = sw.KEYS, sw.WKEYS
SKY_KEYS = ("sky_coef", "sky_cov", "sky_status", "sky_npix")


class OracleContext(sw.OracleContext):
    def scene_fit_flux_sky(self, stamps, places, data_fields, field_ptr=None, sky_order=0, weight_fields=None, min_pivot=1e-8,
                           scratch_bytes=256 << 20):
        stamps = np.asarray(stamps, dtype=np.float32)
        data = np.asarray(data_fields, dtype=np.float64)
        n = len(stamps)
        self.calls.append(dict(fit_flux_sky=n, fields=data.shape[0], sky_order=sky_order, min_pivot=min_pivot,
                               weights=None if weight_fields is None else np.shape(weight_fields),
                               field_ptr=None if field_ptr is None else list(field_ptr)))
        out, _ = fs.fit_flux_sky(stamps, places, [0, n] if field_ptr is None else field_ptr, data, sky_order, weight_fields,
                                 min_pivot)
        return {k: out[k] for k in (KEYS if weight_fields is None else WKEYS) + SKY_KEYS}


def stub_sky(M, nb, q, F):
    """Per-field arrays that encode the field: sky_coef[m, b, t] = 0.1 (m + 1) + 0.01 b + (0.5 if t else 0), sky_cov = diag(0.04,
    0.01, 0.0025)[:q] + 0.001 off the diagonal, sky_npix = F F; field 1 has no counting pixel in the last band (status 4: NaN),
    and at q = 3 field 2 has dropped term 1 of band 0 (status 5: coefficient 0.0, NaN in its row and column)"""
    m, b, t = np.arange(M)[:, None, None], np.arange(nb)[None, :, None], np.arange(q)[None, None, :]
    coef = 0.1 * (m + 1) + 0.01 * b + 0.5 * (t > 0)
    cov = np.tile(np.diag([0.04, 0.01, 0.0025][:q]) + 0.001 * (1 - np.eye(q)), (M, nb, 1, 1))
    status = np.zeros((M, nb, q), np.int32)
    npix = np.full((M, nb), F * F, np.int64)
    if M > 1:
        status[1, -1], coef[1, -1], cov[1, -1], npix[1, -1] = 4, np.nan, np.nan, 0
    if M > 2 and q == 3:
        status[2, 0, 1], coef[2, 0, 1] = 5, 0.0
        cov[2, 0, 1, :] = cov[2, 0, :, 1] = np.nan
    return dict(sky_coef=coef, sky_cov=cov, sky_status=status, sky_npix=npix)


class RecordingEngine(sw.RecordingEngine):
    def infer_fields_measure_fit_sky(self, fields, starts, field_ptr, places, sky_order=0, weight_fields=None, seed=0, band=2,
                                     sigma0=3.0, tol=1e-10, max_iter=200, min_pivot=1e-8, scratch_bytes=256 << 20,
                                     return_fields=True, residual=True, mse_center=True):
        out = self.infer_fields_measure(fields, starts, field_ptr, places=places if return_fields else None, seed=seed,
                                        return_fields=return_fields)
        self.calls.pop(-1)
        self.calls.append(("infer_fields_measure_fit_sky", seed, return_fields, None if places is None else np.array(places),
                           sky_order, None if weight_fields is None else np.asarray(weight_fields)))
        f = sw.stub_fit_flux_weighted(len(starts), fields.shape[3])
        out.update({k: f[k] for k in (KEYS if weight_fields is None else WKEYS)})
        out.update(stub_sky(fields.shape[0], fields.shape[3], 1 if sky_order == 0 else 3, fields.shape[1]))
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
