"""CPU checks of the position fit inside the on-device many-field call (dv_infer_fields_fit_composite): the
entry point in the header, the library and the ctypes table; what DeblendFieldBatch.deblend_fields(optimise_positions=True)
asks of the engine in both modes and what it leaves in the recarrays; the refusals that come before the engine.  The engine
is a stand-in that records its calls, in the manner of tests/test_fields_batch_host.py: no GPU is touched."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, CS, NB = 81, 59, 6
NAME = "dv_infer_fields_fit_composite"


class RecordingEngine:
    def __init__(self):
        self.calls = []

    def set_normalise(self, on):
        self.calls.append(("set_normalise", bool(on)))

    def infer_fields_keep(self, fields, starts, field_ptr, seed=0, want=("loc", "scale")):
        self.calls.append(("infer_fields_keep", np.array(starts), np.array(field_ptr), seed))
        n = len(starts)
        fld = np.repeat(np.arange(len(field_ptr) - 1), np.diff(field_ptr))
        cut = np.stack([fields[f, x:x + CS, y:y + CS] for f, (x, y) in zip(fld, starts)]) if n else np.zeros((0, CS, CS, NB))
        loc = np.zeros((n, CS, CS, NB), np.float32) + np.arange(n, dtype=np.float32)[:, None, None, None]
        return {"loc": loc, "scale": loc + 0.5, "cutouts": cut}

    def infer_fields_composite(self, fields, starts, places, field_ptr, seed=0, residual=True, mse_center=True):
        self.calls.append(("infer_fields_composite", np.array(starts), np.array(places), np.array(field_ptr), seed))
        return {"mean_fields": np.full(fields.shape, 1.0), "stddev_fields": np.full(fields.shape, 2.0),
                "residual_fields": fields - 1.0, "mse_center": np.arange(len(starts), dtype=np.float64) * 60.0}

    def infer_fields_fit_composite(self, fields, starts, distances, field_ptr, seed=0, shifts=None, bound=3.0, max_iter=50,
                                   mc_seed=0, nsamples=0, residual=True, mse_center=True):
        self.calls.append(("infer_fields_fit_composite", np.array(starts), np.array(distances), np.array(field_ptr), seed,
                           shifts, bound, max_iter, mc_seed, nsamples))
        n = len(starts)
        out = {"mean_fields": np.full(fields.shape, 1.0), "stddev_fields": np.full(fields.shape, 2.0),
               "residual_fields": fields - 1.0, "mse_center": np.arange(n, dtype=np.float64) * 60.0,
               "shifts": np.stack([np.arange(n) + 0.25, -np.arange(n) - 0.5], axis=1), "objective": np.arange(n) * 2.0,
               "iters": np.arange(n, dtype=np.int32) + 3, "status": np.arange(n, dtype=np.int32) % 4}
        if nsamples:
            out["epistemic_fields"] = np.full(fields.shape, 3.0)
            out["eps_norm"] = np.arange(n, dtype=np.float64)
        return out


class Core:
    def __init__(self):
        self.engine, self.ctx, self.seed_counter = RecordingEngine(), None, 7

    def next_seed(self):
        self.seed_counter += 1
        return self.seed_counter


class Net:
    def __init__(self):
        self._core = Core()


def _fields(m=4):
    return np.random.default_rng(3).normal(size=(m, F, F, NB))


# distances per field: two valid, none, one valid + one off the field, only invalid ones
DIST = [np.array([[0.0, 0.0], [5.0, -7.0]]), np.zeros((0, 2)), np.array([[100.0, 0.0], [-3.0, 11.0]]),
        np.array([[0.0, 40.0]])]


def test_entry_point_in_header_library_and_ctypes_table():
    from debvader_amd import _lib

    header = open(os.path.join(ROOT, "include", "debvader_hip.h")).read()
    decl = re.search(r"int " + NAME + r"\(([^;]*)\);", header)
    assert decl is not None
    params = [p.strip() for p in decl.group(1).replace("\n", " ").split(",")]
    restype, argtypes = _lib.SIGNATURES[NAME]
    assert len(params) == len(argtypes) == 24
    for word in ("dist", "bound", "max_iter", "shifts_inout", "mc_seed", "nsamples", "objective", "iters", "status"):
        assert any(p.endswith(word) for p in params), word
    assert hasattr(_lib.lib, NAME) and getattr(_lib.lib, NAME).argtypes == argtypes
    # nothing but dv_* leaves the library: the version script needs no new line for it
    assert "dv_*" in open(os.path.join(ROOT, "debvader_amd", "csrc", "exports.map")).read()


def test_wrapper_signatures():
    from debvader_amd import engine as E
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch

    p = inspect.signature(E.Engine.infer_fields_fit_composite).parameters
    assert list(p)[:5] == ["self", "fields", "starts", "distances", "field_ptr"]
    assert p["bound"].default == 3.0 and p["max_iter"].default == 50 and p["nsamples"].default == 0
    assert "distances" in inspect.signature(E.Engine.infer_cutouts_fit_composite).parameters
    p = inspect.signature(DeblendFieldBatch.deblend_fields).parameters
    assert list(p)[-1] == "optimise_positions" and p["optimise_positions"].default is False


def test_on_device_fit_is_one_engine_call():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch

    net = Net()
    db = DeblendFieldBatch(net, _fields())
    res = db.deblend_fields(DIST, on_device=True, optimise_positions=True)
    calls = net._core.engine.calls
    assert [c[0] for c in calls] == ["set_normalise", "infer_fields_fit_composite", "set_normalise"]
    _, starts, dist, fp, seed, shifts, bound, max_iter, mc_seed, nsamples = calls[1]
    assert np.array_equal(dist, np.array([[0.0, 0.0], [5.0, -7.0], [-3.0, 11.0]])) and fp.tolist() == [0, 2, 2, 3, 3]
    assert len(starts) == 3 and seed == 8 and shifts is None and bound == 3.0 and max_iter == 50 and nsamples == 0
    assert [r.dtype.names for r in res] == [tuple(n for n, _ in DeblendFieldBatch.ON_DEVICE_COLUMNS)] * 4
    assert [len(r) for r in res] == [2, 0, 1, 0]
    got = [s for r in res for s in r["shifts"]]
    assert all(s.dtype == np.float64 and s.shape == (2,) for s in got)
    assert np.array_equal(np.array(got), np.array([[0.25, -0.5], [1.25, -1.5], [2.25, -2.5]]))
    assert len(db.position_fit) == 4 and sorted(db.position_fit[0]) == ["iters", "objective", "status"]
    assert db.position_fit[0]["iters"].tolist() == [3, 4] and db.position_fit[2]["objective"].tolist() == [4.0]
    assert db.position_fit[1]["status"].shape == (0,) and db.position_fit[2]["status"].tolist() == [2]
    assert res[0]["passed_cuts"].tolist() == [True, True] and res[2]["passed_cuts"].tolist() == [False]
    # the fields are the device-composited ones
    assert np.array_equal(db.get_predicted_fields()["predicted_mean_fields"], np.full(db.field_images.shape, 1.0))
    assert np.array_equal(db.get_residual_fields(), db.field_images - 1.0)

    # with the epistemic estimate: the pass's seed, then the Monte-Carlo stage's, as without the fit
    net = Net()
    db = DeblendFieldBatch(net, _fields())
    res = db.deblend_fields(DIST, on_device=True, epistemic_uncertainty_estimation=True, epistemic_samples=5,
                            optimise_positions=True)
    c = net._core.engine.calls[1]
    assert c[0] == "infer_fields_fit_composite" and (c[4], c[8], c[9]) == (8, 9, 5)
    assert [r.dtype.names for r in res] == [tuple(n for n, _ in DeblendFieldBatch.ON_DEVICE_EPISTEMIC_COLUMNS)] * 4
    assert "predicted_epistemic_fields" in db.get_predicted_fields()


def test_without_the_keyword_the_call_lists_are_unchanged():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch

    for kw in ({}, {"optimise_positions": False}):
        net = Net()
        db = DeblendFieldBatch(net, _fields())
        db.deblend_fields(DIST, on_device=True, **kw)
        calls = net._core.engine.calls
        assert [c[0] for c in calls] == ["set_normalise", "infer_fields_composite", "set_normalise"] and calls[1][4] == 8
        assert db.position_fit is None and all(np.array_equal(s, [0, 0]) for r in db.res_deblend for s in r["shifts"])
        net = Net()
        db = DeblendFieldBatch(net, _fields())
        db.deblend_fields(DIST, **kw)
        calls = net._core.engine.calls
        assert [c[0] for c in calls] == ["set_normalise", "infer_fields_keep", "set_normalise"] and calls[1][3] == 8


def test_default_path_fit_is_the_pass_followed_by_optimise_positions(monkeypatch):
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch

    net = Net()
    db = DeblendFieldBatch(net, _fields())
    seen = []
    monkeypatch.setattr(DeblendFieldBatch, "optimise_positions", lambda self: seen.append(len(self.res_deblend)))
    res = db.deblend_fields(DIST, optimise_positions=True)
    assert seen == [4] and res is db.res_deblend
    assert [c[0] for c in net._core.engine.calls] == ["set_normalise", "infer_fields_keep", "set_normalise"]


def test_refusals_come_before_the_engine():
    from debvader_amd import engine as E
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch

    net = Net()
    db = DeblendFieldBatch(net, _fields())
    with pytest.raises(ValueError, match="integer"):
        db.deblend_fields([d + 0.5 for d in DIST], on_device=True, optimise_positions=True)
    assert net._core.engine.calls == []
    two = DeblendFieldBatch(Net(), np.zeros((1, F, F, 2)), nb_of_bands=2)
    with pytest.raises(ValueError, match="band 2"):
        two.deblend_fields([np.zeros((1, 2))], on_device=True, optimise_positions=True)
    assert two.net._core.engine.calls == []
    # the unbound method validates before it touches self._h: a bare object stands in for the engine
    f, st, d, fp = np.zeros((1, F, F, NB)), [[11, 11]], [[0.0, 0.0]], [0, 1]
    call = E.Engine.infer_fields_fit_composite
    with pytest.raises(ValueError, match="integer distances"):
        call(object(), f, st, [[0.5, 0.0]], fp)
    with pytest.raises(ValueError, match="integer distances"):
        call(object(), f, st, [[np.nan, 0.0]], fp)
    with pytest.raises(ValueError, match="band 2"):
        call(object(), np.zeros((1, F, F, 2)), st, d, fp)
    for bad in (dict(bound=-1.0), dict(bound=np.inf), dict(bound=np.nan), dict(max_iter=-1)):
        with pytest.raises(ValueError, match="bound must"):
            call(object(), f, st, d, fp, **bad)
    with pytest.raises(ValueError, match="start shifts"):
        call(object(), f, st, d, fp, shifts=[[np.inf, 0.0]])
    with pytest.raises(ValueError, match="start shifts"):
        call(object(), f, st, d, fp, shifts=[[0.0, 0.0], [1.0, 1.0]])
    with pytest.raises(ValueError, match="distances of shape"):
        call(object(), f, st, [[0.0, 0.0], [1.0, 1.0]], fp)
    with pytest.raises(ValueError, match="nsamples"):
        call(object(), f, st, d, fp, nsamples=-2)
    with pytest.raises(ValueError, match="field_ptr"):
        call(object(), f, st, d, [0, 2])
    with pytest.raises(ValueError, match="square field"):
        E.Engine.infer_cutouts_fit_composite(object(), np.zeros((F, F + 1, NB)), st, d)
