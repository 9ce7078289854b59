"""Stand-ins for the engine and its context in the CPU tests of the flux fit by blend groups
(tests/test_fit_flux_groups_host.py), in the manner of tests/stub_fit_flux_engine.py: no GPU, no HIP.  The context answers
scene_fit_flux_groups with the numpy restatement of tests/fit_flux_groups_oracle.py; the engine records its calls and returns
rows that encode the global stamp number."""
import numpy as np

from tests import fit_flux_groups_oracle as go
from tests import stub_fit_flux_weighted_engine as sw

CS, NB = sw.CS, sw.NB
KEYS, WKEYS = sw.KEYS, sw.WKEYS
GKEYS = ("fit_group", "fit_group_size")


class OracleContext(sw.OracleContext):
    def scene_fit_flux_groups(self, stamps, places, data_fields, field_ptr=None, min_pivot=1e-8, scratch_bytes=256 << 20,
                              weight_fields=None):
        stamps = np.asarray(stamps, dtype=np.float32)
        data = np.asarray(data_fields, dtype=np.float64)
        n = len(stamps)
        self.calls.append(dict(fit_flux_groups=n, fields=data.shape[0], min_pivot=min_pivot,
                               weights=None if weight_fields is None else np.shape(weight_fields),
                               field_ptr=None if field_ptr is None else list(field_ptr)))
        out, _ = go.fit_flux_groups(stamps, places, [0, n] if field_ptr is None else field_ptr, data,
                                    None if weight_fields is None else np.asarray(weight_fields, dtype=np.float64), min_pivot)
        return {k: out[k] for k in (KEYS if weight_fields is None else WKEYS) + GKEYS}


def stub_fit_groups(n):
    """Rows that encode their number: fit_group = i - i % 3, fit_group_size = 1 + i % 4"""
    i = np.arange(n)
    return dict(fit_group=(i - i % 3).astype(np.int32), fit_group_size=(1 + i % 4).astype(np.int32))


class RecordingEngine(sw.RecordingEngine):
    def infer_fields_measure_fit_groups(self, fields, starts, field_ptr, places, weight_fields=None, seed=0, band=2, sigma0=3.0,
                                        tol=1e-10, max_iter=200, min_pivot=1e-8, scratch_bytes=256 << 20, return_fields=True,
                                        residual=True, mse_center=True):
        out = self.infer_fields_measure(fields, starts, field_ptr, places=places if return_fields else None, seed=seed,
                                        return_fields=return_fields)
        self.calls.pop(-1)
        self.calls.append(("infer_fields_measure_fit_groups", seed, return_fields, None if places is None else np.array(places),
                           None if weight_fields is None else np.asarray(weight_fields)))
        n, nb = len(starts), fields.shape[3]
        out.update(sw.sf.stub_fit_flux(n, nb) if weight_fields is None else sw.stub_fit_flux_weighted(n, nb))
        out.update(stub_fit_groups(n))
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
