"""Stand-ins for the engine and its context in the CPU tests of the measurement layer (tests/test_measure_host.py), in the
manner of tests/stub_engine.py: no GPU, no HIP.  The context measures with the numpy oracle; the engine records its calls
and returns stamps and catalogues that encode the global stamp number."""
import numpy as np

from tests import measure_oracle as mo

CS, NB = 59, 6


class OracleContext:
    """Context.scene_measure answered by tests/measure_oracle.py"""

    def __init__(self):
        self.calls = []

    def scene_measure(self, mean, stddev=None, band=2, sigma0=3.0, tol=1e-10, max_iter=200):
        self.calls.append(dict(n=len(mean), band=band, sigma0=sigma0, tol=tol, max_iter=max_iter, dtype=mean.dtype,
                               with_stddev=stddev is not None))
        out = mo.measure(mean, stddev, band, sigma0, tol, max_iter)
        if stddev is None:
            del out["flux_err"]
        return out


def stub_catalogue(n, nb=NB):
    """A catalogue whose row i encodes i; every third row failed"""
    i = np.arange(n, dtype=np.float64)
    shape = np.stack([29.0 + 0.25 * i, 29.0 - 0.5 * i, 4.0 + i, 0.5 * np.ones(n), 9.0 + i], axis=1).reshape(n, 5)
    return dict(flux=i[:, None] + np.arange(nb)[None, :], flux_err=0.1 * (i[:, None] + 1) * np.ones((1, nb)), shape=shape,
                iters=(20 + np.arange(n)).astype(np.int32), status=np.where(np.arange(n) % 3 == 2, 3, 0).astype(np.int32))


class RecordingEngine:
    def __init__(self):
        self.calls = []

    def set_normalise(self, on):
        self.calls.append(("set_normalise", bool(on)))

    def infer_fields_keep(self, fields, starts, field_ptr, seed=0, want=("loc", "scale")):
        self.calls.append(("infer_fields_keep", seed))
        n = len(starts)
        fld = np.repeat(np.arange(len(field_ptr) - 1), np.diff(field_ptr))
        cut = np.stack([fields[f, x:x + CS, y:y + CS] for f, (x, y) in zip(fld, starts)]) if n else np.zeros((0, CS, CS, NB))
        # a round blob per stamp, offset by the stamp number: something the oracle can measure
        loc = np.stack([mo.gaussian_stamp(CS, (5.0, 0.0, 5.0), (0.5 * i, -0.25 * i))[:, :, None] * np.ones(NB)
                        for i in range(n)]).astype(np.float32) if n else np.zeros((0, CS, CS, NB), np.float32)
        return {"loc": loc, "scale": np.full_like(loc, 0.5), "cutouts": cut}

    def infer_fields_composite(self, fields, starts, places, field_ptr, seed=0, residual=True, mse_center=True):
        self.calls.append(("infer_fields_composite", seed))
        return {"mean_fields": np.full(fields.shape, 1.0), "stddev_fields": np.full(fields.shape, 2.0),
                "residual_fields": fields - 1.0, "mse_center": np.arange(len(starts), dtype=np.float64) * 60.0}

    def infer_fields_measure(self, fields, starts, field_ptr, places=None, seed=0, band=2, sigma0=3.0, tol=1e-10,
                             max_iter=200, return_fields=True, residual=True, mse_center=True):
        self.calls.append(("infer_fields_measure", seed, return_fields, None if places is None else np.array(places)))
        out = self.infer_fields_composite(fields, starts, places, field_ptr, seed) if return_fields else \
            {"mse_center": np.arange(len(starts), dtype=np.float64) * 60.0}
        self.calls.pop(-1) if return_fields else None
        out.update(stub_catalogue(len(starts), fields.shape[3]))
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
