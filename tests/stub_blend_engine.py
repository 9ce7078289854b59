"""Stand-ins for the engine and its context in the CPU tests of the blendedness layer (tests/test_blend_host.py), in the
manner of tests/stub_measure_engine.py: no GPU, no HIP.  The context answers scene_blend with the numpy restatement; the
engine records its calls and returns blend rows that encode the global stamp number."""
import numpy as np

from tests import blend_oracle as bo
from tests import stub_measure_engine as sm

CS, NB = sm.CS, sm.NB


class OracleContext(sm.OracleContext):
    """Context.scene_blend answered by tests/blend_oracle.py"""

    def scene_blend(self, stamps, shape, status, places, model_fields, data_fields=None, field_ptr=None, band=2):
        self.calls.append(dict(n=len(stamps), band=band, with_data=data_fields is not None,
                               field_ptr=None if field_ptr is None else list(field_ptr), fields=np.shape(model_fields)))
        out = bo.blend(stamps, shape, status, places, model_fields, data_fields, field_ptr, band)
        return dict(blend=out["blend"], npix=out["npix"])


def stub_blend(n):
    """Rows that encode i: {W, A, Bm, Bd} = {10 + i, 2 + i, 4 + 2 i, 8 + i}; row 1 has Bm = 0, row 2 is ineligible (as
    stub_catalogue's status 3), row 3 has Bd < 0, row 4 has npix 0 with four zero sums"""
    i = np.arange(n, dtype=np.float64)
    blend = np.stack([10.0 + i, 2.0 + i, 4.0 + 2.0 * i, 8.0 + i], axis=1).reshape(n, 4)
    npix = np.full(n, CS * CS, np.int32)
    if n > 1:
        blend[1, 2] = 0.0
    if n > 2:
        blend[2], npix[2] = np.nan, -1
    if n > 3:
        blend[3, 3] = -1.0
    if n > 4:
        blend[4], npix[4] = 0.0, 0
    return dict(blend=blend, npix=npix)


class RecordingEngine(sm.RecordingEngine):
    def infer_fields_measure_blend(self, fields, starts, field_ptr, places, seed=0, band=2, sigma0=3.0, tol=1e-10,
                                   max_iter=200, return_fields=True, residual=True, mse_center=True):
        out = self.infer_fields_measure(fields, starts, field_ptr, places=places, seed=seed, return_fields=return_fields)
        self.calls[-1] = ("infer_fields_measure_blend",) + self.calls[-1][1:]
        out.update(stub_blend(len(starts)))
        return out


class Core(sm.Core):
    def __init__(self):
        super().__init__()
        self.engine, self.ctx = RecordingEngine(), OracleContext()


class Net:
    def __init__(self):
        self._core = Core()
