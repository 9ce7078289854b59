"""Stand-ins for the engine and its context in the CPU tests of the apertures on the fields
(tests/test_aperture_fields_host.py), in the manner of tests/stub_aperture_engine.py: no GPU, no HIP.  The context answers
scene_measure, scene_aperture and scene_aperture_fields with the numpy restatements; the engine records its calls and returns
rows that encode the global stamp number."""
import numpy as np

from tests import aperture_fields_oracle as afo
from tests import stub_aperture_engine as sa

CS, NB = sa.CS, sa.NB


class OracleContext(sa.OracleContext):
    def scene_aperture_fields(self, shape, status, places, kron, aper_status, model_fields, data_fields=None, field_ptr=None, *,
                              cutout_size, radii=(3.0, 5.0, 8.0), subsample=5):
        model = np.asarray(model_fields, dtype=np.float64)
        n, nb, K = len(status), model.shape[3], len(tuple(radii))
        self.calls.append(dict(aperture_fields=n, radii=tuple(radii), subsample=subsample, cutout_size=cutout_size,
                               with_data=data_fields is not None, field_ptr=None if field_ptr is None else list(field_ptr)))
        fp = [0, n] if field_ptr is None else field_ptr
        rows = afo.aperture_fields(shape, status, aper_status, kron, places, fp, model, data_fields, cutout_size,
                                   afo.params(radii=tuple(radii), subsample=subsample), shortcut=True)
        tails = dict(ap_model_sum=(K, nb), ap_data_sum=(K, nb), ap_field_area=(K,), auto_model_sum=(nb,), auto_data_sum=(nb,),
                     auto_field_area=())
        return {k: np.array([r[k] for r in rows], dtype=np.float64).reshape((n,) + t) for k, t in tails.items()}


def stub_aperture_fields(n, nb, K):
    """Rows that go with stub_aperture's and encode their number: ap_model_sum = 1.25 ap_flux, ap_data_sum = ap_model_sum + 2,
    ap_field_area = ap_area but for circle 0 of row 2 (one less), auto_model_sum = 2 flux_auto, auto_data_sum =
    auto_model_sum - 0.5, auto_field_area = auto_area but for row 3 (half); NaN where stub_aperture's are"""
    s = sa.stub_aperture(n, nb, K, 0)
    out = dict(ap_model_sum=1.25 * s["ap_flux"], ap_data_sum=1.25 * s["ap_flux"] + 2.0, ap_field_area=s["ap_area"].copy(),
               auto_model_sum=2.0 * s["flux_auto"], auto_data_sum=2.0 * s["flux_auto"] - 0.5,
               auto_field_area=s["kron"][:, 2].copy())
    if n > 2 and K:
        out["ap_field_area"][2, 0] -= 1.0
    if n > 3:
        out["auto_field_area"][3] *= 0.5
    return out


class RecordingEngine(sa.RecordingEngine):
    def infer_fields_measure_aper_data(self, fields, starts, field_ptr, places, seed=0, band=2, sigma0=3.0, tol=1e-10,
                                       max_iter=200, radii=(3.0, 5.0, 8.0), fractions=(0.2, 0.5, 0.8), subsample=5,
                                       kron_factor=2.5, kron_min=3.5, kron_limit=6.0, bisect_iters=32, return_fields=True,
                                       residual=True, mse_center=True):
        out = self.infer_fields_measure_aper(fields, starts, field_ptr, places=places if return_fields else None, seed=seed,
                                             radii=radii, fractions=fractions, return_fields=return_fields)
        self.calls.pop(-1)
        self.calls.append(("infer_fields_measure_aper_data", seed, return_fields, None if places is None else np.array(places),
                           tuple(radii), tuple(fractions)))
        out.update(stub_aperture_fields(len(starts), fields.shape[3], len(radii)))
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
