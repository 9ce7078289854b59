"""CPU checks of the epistemic estimate in the on-device and many-field deblending calls: the two
C-ABI entry points, the seeds and the sample count the classes hand to the engine, the cut that combines both criteria, the
recarray columns, and that a pass without the estimate makes exactly the engine calls it made before.  The engine is a
stand-in that records its calls, in the manner of tests/test_fields_batch_host.py: no GPU is touched."""
import os
import re

import numpy as np
import pytest

F, CS, NB = 81, 59, 6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class RecordingEngine:
    """Stamps that encode their global stamp number; eps_norm = 50 * (stamp number + 1), mse_center = 60 * stamp number."""

    def __init__(self):
        self.calls = []

    def set_normalise(self, on):
        self.calls.append(("set_normalise", bool(on)))

    def _stamps(self, fields, starts, field_ptr):
        n = len(starts)
        fld = np.repeat(np.arange(len(field_ptr) - 1), np.diff(field_ptr))
        cut = np.stack([fields[f, x:x + CS, y:y + CS] for f, (x, y) in zip(fld, starts)]) if n else np.zeros((0, CS, CS, NB))
        loc = np.zeros((n, CS, CS, NB), np.float32) + np.arange(n, dtype=np.float32)[:, None, None, None] + 1.0
        return {"loc": loc, "scale": loc + 0.5, "cutouts": cut}

    def infer_fields_keep(self, fields, starts, field_ptr, seed=0, want=("loc", "scale")):
        self.calls.append(("infer_fields_keep", np.array(starts), np.array(field_ptr), seed))
        return self._stamps(fields, starts, field_ptr)

    def infer_fields_composite(self, fields, starts, places, field_ptr, seed=0, residual=True, mse_center=True):
        self.calls.append(("infer_fields_composite", np.array(starts), np.array(places), np.array(field_ptr), seed))
        return {"mean_fields": np.full(fields.shape, 1.0), "stddev_fields": np.full(fields.shape, 2.0),
                "residual_fields": fields - 1.0, "mse_center": np.arange(len(starts), dtype=np.float64) * 60.0}

    def infer_fields_mc_keep(self, fields, starts, field_ptr, seed=0, mc_seed=0, nsamples=100):
        self.calls.append(("infer_fields_mc_keep", np.array(starts), np.array(field_ptr), seed, mc_seed, nsamples))
        out = self._stamps(fields, starts, field_ptr)
        # std stamps whose band-2 sum is 50 * (i + 1) times the band-2 sum of the mean
        out["epistemic"] = (out["loc"] * (50.0 * (np.arange(len(starts), dtype=np.float32) + 1.0))[:, None, None, None])
        return out

    def infer_fields_mc_composite(self, fields, starts, places, field_ptr, seed=0, mc_seed=0, nsamples=100, residual=True,
                                  mse_center=True):
        self.calls.append(("infer_fields_mc_composite", np.array(starts), np.array(places), np.array(field_ptr), seed,
                           mc_seed, nsamples))
        n = len(starts)
        return {"mean_fields": np.full(fields.shape, 1.0), "stddev_fields": np.full(fields.shape, 2.0),
                "epistemic_fields": np.full(fields.shape, 3.0), "residual_fields": fields - 1.0,
                "mse_center": np.arange(n, dtype=np.float64) * 60.0, "eps_norm": 50.0 * (np.arange(n, dtype=np.float64) + 1.0)}

    # the single-field forms DeblendField calls
    def infer_cutouts_mc_keep(self, field, starts, seed=0, mc_seed=0, nsamples=100):
        self.calls.append(("infer_cutouts_mc_keep", np.array(starts), seed, mc_seed, nsamples))
        out = self._stamps(field[None], starts, [0, len(starts)])
        out["epistemic"] = (out["loc"] * (50.0 * (np.arange(len(starts), dtype=np.float32) + 1.0))[:, None, None, None])
        return out

    def infer_cutouts_mc_composite(self, field, starts, places, seed=0, mc_seed=0, nsamples=100, residual=True,
                                   mse_center=True):
        self.calls.append(("infer_cutouts_mc_composite", np.array(starts), np.array(places), seed, mc_seed, nsamples))
        n = len(starts)
        return {"mean_field": np.full(field.shape, 1.0), "stddev_field": np.full(field.shape, 2.0),
                "epistemic_field": np.full(field.shape, 3.0), "residual_field": field - 1.0,
                "mse_center": np.arange(n, dtype=np.float64) * 60.0, "eps_norm": 50.0 * (np.arange(n, dtype=np.float64) + 1.0)}


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


# distances per field: two valid, none, one valid + one off the field, only invalid ones (test_fields_batch_host.py's)
DIST = [np.array([[0.0, 0.0], [5.0, -7.0]]), np.zeros((0, 2)), np.array([[100.0, 0.0], [-3.0, 11.0]]),
        np.array([[0.0, 40.0]])]
NEW = ("dv_infer_fields_mc_keep", "dv_infer_fields_mc_composite")


def _c_types(arglist):
    """The parameter types of a C prototype's argument list, without names and qualifiers"""
    out = []
    for a in arglist.split(","):
        a = re.sub(r"/\*.*?\*/", "", a).replace("const", "").strip()
        out.append(re.sub(r"\s*\w+$", "", a).replace(" ", ""))
    return out


def test_header_declares_and_the_library_exports_the_new_entry_points():
    import ctypes as C

    from debvader_amd import _lib

    header = open(os.path.join(ROOT, "include", "debvader_hip.h")).read()
    ctype = {"dv_model*": C.c_void_p, "double*": C.POINTER(C.c_double), "float*": C.POINTER(C.c_float),
             "int32_t*": C.POINTER(C.c_int32), "int64_t*": C.POINTER(C.c_int64), "int32_t": C.c_int32, "int64_t": C.c_int64,
             "uint64_t": C.c_uint64}
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header, re.S)
        assert m, f"{name} is not declared in include/debvader_hip.h"
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)         # bound: the library exports it
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int
        want = [ctype[t] for t in _c_types(m.group(1))]
        assert len(argtypes) == len(want)
        for i, (a, w) in enumerate(zip(argtypes, want)):
            assert a is w or (w is C.c_void_p and a in (C.c_void_p, _lib.SIGNATURES["dv_infer_fields"][1][0])), (name, i, a, w)
    assert len(_lib.SIGNATURES["dv_infer_fields_mc_keep"][1]) == 15
    assert len(_lib.SIGNATURES["dv_infer_fields_mc_composite"][1]) == 18
    # exports.map lets every dv_* symbol through and nothing else: the two new names need no line of their own
    emap = open(os.path.join(ROOT, "debvader_amd", "csrc", "exports.map")).read()
    assert "global: dv_*;" in emap and "local: *;" in emap


def test_engine_wrappers_refuse_before_the_library_is_touched():
    from debvader_amd import engine as E

    f = np.zeros((1, F, F, NB))
    for name in ("infer_fields_mc_keep", "infer_fields_mc_composite", "infer_cutouts_mc_keep", "infer_cutouts_mc_composite"):
        assert hasattr(E.Engine, name)
    # the unbound methods validate before they touch self._h: a bare object stands in for the engine
    with pytest.raises(ValueError, match="nsamples"):
        E.Engine.infer_fields_mc_keep(object(), f, [[0, 0]], [0, 1], nsamples=0)
    with pytest.raises(ValueError, match="band 2"):
        E.Engine.infer_fields_mc_keep(object(), f[..., :2], [[0, 0]], [0, 1])
    with pytest.raises(ValueError, match="nsamples"):
        E.Engine.infer_fields_mc_composite(object(), f, [[0, 0]], [[0, 0]], [0, 1], nsamples=-3)
    with pytest.raises(ValueError, match="band 2"):
        E.Engine.infer_fields_mc_composite(object(), f[..., :2], [[0, 0]], [[0, 0]], [0, 1])
    with pytest.raises(ValueError, match="field_ptr"):
        E.Engine.infer_fields_mc_keep(object(), f, [[0, 0]], [0, 2])
    with pytest.raises(ValueError, match="placements"):
        E.Engine.infer_fields_mc_composite(object(), f, [[0, 0]], [[0, 0], [1, 1]], [0, 1])


def test_batch_on_device_pass_with_the_estimate():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch

    net, fields = Net(), _fields()
    db = DeblendFieldBatch(net, fields, cutout_size=CS, nb_of_bands=NB, normalise=True)
    res = db.deblend_fields(DIST, on_device=True, epistemic_uncertainty_estimation=True)
    eng = net._core.engine
    assert [c[0] for c in eng.calls] == ["set_normalise", "infer_fields_mc_composite", "set_normalise"]
    assert eng.calls[0][1] is True and eng.calls[2][1] is False
    _, starts, places, fp, seed, mc_seed, nsamples = eng.calls[1]
    assert (seed, mc_seed) == (8, 9) and net._core.seed_counter == 9       # two consecutive seeds: pass, then Monte Carlo
    assert nsamples == 100 and fp.tolist() == [0, 2, 2, 3, 3]
    po = int((F - CS) / 2)
    assert np.array_equal(places, po + np.array([[0, 0], [5, -7], [-3, 11]]))
    want = [("list_idx", "int64"), ("shifts", "object"), ("galaxy_distances_to_center_x", "float64"),
            ("galaxy_distances_to_center_y", "float64"), ("mse_center", "float64"), ("epistemic_norm", "float64"),
            ("passed_cuts", "bool")]
    for r in res:
        assert isinstance(r, np.recarray)
        assert [(k, str(r.dtype[k])) for k in r.dtype.names] == want
    # eps_norm 50, 100 | 150 and mse_center 0, 60 | 120 against the default criteria of 100: only stamp 0 passes both
    assert res[0]["epistemic_norm"].tolist() == [50.0, 100.0] and res[2]["epistemic_norm"].tolist() == [150.0]
    assert res[0]["passed_cuts"].tolist() == [True, True] and res[2]["passed_cuts"].tolist() == [False]
    pred = db.get_predicted_fields()
    assert sorted(pred) == ["predicted_epistemic_fields", "predicted_mean_fields", "predicted_stddev_fields"]
    assert (pred["predicted_epistemic_fields"] == 3.0).all() and pred["predicted_epistemic_fields"].shape == fields.shape
    # each criterion cuts on its own
    res = db.deblend_fields(DIST, on_device=True, epistemic_uncertainty_estimation=True, epistemic_criterion=60.0,
                            mse_criterion=1e9, epistemic_samples=12)
    assert eng.calls[-2][-1] == 12 and (eng.calls[-2][-3], eng.calls[-2][-2]) == (10, 11)
    assert res[0]["passed_cuts"].tolist() == [True, False] and res[2]["passed_cuts"].tolist() == [False]
    res = db.deblend_fields(DIST, on_device=True, epistemic_uncertainty_estimation=True, epistemic_criterion=1e9,
                            mse_criterion=30.0)
    assert res[0]["passed_cuts"].tolist() == [True, False] and res[2]["passed_cuts"].tolist() == [False]
    res = db.deblend_fields(DIST, on_device=True, epistemic_uncertainty_estimation=True, epistemic_criterion=120.0,
                            mse_criterion=90.0)
    assert res[0]["passed_cuts"].tolist() == [True, True] and res[2]["passed_cuts"].tolist() == [False]


def test_batch_default_pass_with_the_estimate():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch

    net, fields = Net(), _fields()
    net._core.ctx = None
    db = DeblendFieldBatch(net, fields, cutout_size=CS, nb_of_bands=NB)
    res = db.deblend_fields(DIST, mse_criterion=1.0e9, epistemic_uncertainty_estimation=True, epistemic_criterion=120.0)
    eng = net._core.engine
    assert [c[0] for c in eng.calls] == ["set_normalise", "infer_fields_mc_keep", "set_normalise"]
    assert eng.calls[1][3:] == (8, 9, 100)
    want = [("cutout_images", "object"), ("output_images_mean", "object"), ("output_images_stddev", "object"),
            ("shifts", "object"), ("list_idx", "int64"), ("galaxy_distances_to_center_x", "float64"),
            ("galaxy_distances_to_center_y", "float64"), ("epistemic_uncertainty", "object"), ("passed_cuts", "bool")]
    for r in res:
        assert [(k, str(r.dtype[k])) for k in r.dtype.names] == want          # the default columns, with or without it
    row = res[2][0]                                                            # global stamp 2: mean 3, std stamps 150 * 3
    assert row["epistemic_uncertainty"].dtype == np.float64 and (row["epistemic_uncertainty"] == 450.0).all()
    assert (row["output_images_mean"] == 3.0).all()
    # eps_norm 50, 100 | 150 against 120
    assert res[0]["passed_cuts"].tolist() == [True, True] and res[2]["passed_cuts"].tolist() == [False]


def test_a_pass_without_the_estimate_makes_the_calls_it_made_before():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch

    for kwargs in ({}, {"epistemic_uncertainty_estimation": False, "epistemic_criterion": 1.0, "epistemic_samples": 0}):
        net, fields = Net(), _fields()
        db = DeblendFieldBatch(net, fields, cutout_size=CS, nb_of_bands=NB, normalise=True)
        res = db.deblend_fields(DIST, on_device=True, **kwargs)
        eng = net._core.engine
        assert [c[0] for c in eng.calls] == ["set_normalise", "infer_fields_composite", "set_normalise"]
        assert len(eng.calls[1]) == 5 and eng.calls[1][4] == 8 and net._core.seed_counter == 8      # one seed
        assert [k for k in res[0].dtype.names] == ["list_idx", "shifts", "galaxy_distances_to_center_x",
                                                   "galaxy_distances_to_center_y", "mse_center", "passed_cuts"]
        assert res[0]["passed_cuts"].tolist() == [True, True] and res[2]["passed_cuts"].tolist() == [False]
        assert sorted(db.get_predicted_fields()) == ["predicted_mean_fields", "predicted_stddev_fields"]
        res = db.deblend_fields(DIST, mse_criterion=1.0e9, **kwargs)
        assert [c[0] for c in eng.calls[3:]] == ["set_normalise", "infer_fields_keep", "set_normalise"]
        assert len(eng.calls[4]) == 4 and eng.calls[4][3] == 9
        assert not res[2][0]["epistemic_uncertainty"].any()
    # after a pass with the estimate, a pass without it drops the extra key again
    net = Net()
    db = DeblendFieldBatch(net, _fields(), cutout_size=CS, nb_of_bands=NB)
    db.deblend_fields(DIST, on_device=True, epistemic_uncertainty_estimation=True)
    assert "predicted_epistemic_fields" in db.get_predicted_fields()
    db.deblend_fields(DIST, on_device=True)
    assert sorted(db.get_predicted_fields()) == ["predicted_mean_fields", "predicted_stddev_fields"]


def test_refusals_before_the_engine_is_touched():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch

    net = Net()
    with pytest.raises(TypeError):                       # the estimate is an option of the pass, not of the object
        DeblendFieldBatch(net, _fields(1), epistemic_uncertainty_estimation=True)
    db = DeblendFieldBatch(net, _fields(2), cutout_size=CS, nb_of_bands=NB)
    dist = [np.array([[0.0, 0.0]]), np.zeros((0, 2))]
    for on_device in (False, True):
        with pytest.raises(ValueError, match="epistemic_samples"):
            db.deblend_fields(dist, on_device=on_device, epistemic_uncertainty_estimation=True, epistemic_samples=0)
    two = DeblendFieldBatch(net, _fields(2)[..., :2], cutout_size=CS, nb_of_bands=2)
    for on_device in (False, True):
        with pytest.raises(ValueError, match="band 2"):
            two.deblend_fields(dist, on_device=on_device, epistemic_uncertainty_estimation=True)
    assert net._core.engine.calls == [] and net._core.seed_counter == 7


def test_deblend_field_on_device_with_the_estimate():
    from debvader_amd.deblend.field_deblender import DeblendField

    net, fields = Net(), _fields(1)
    db = DeblendField(net, fields, cutout_size=CS, nb_of_bands=NB, epistemic_uncertainty_estimation=True)
    dist = np.array([[0.0, 0.0], [5.0, -7.0], [-3.0, 11.0]])
    res = db.deblend_field(dist, on_device=True)                    # (raised NotImplementedError before)
    eng = net._core.engine
    assert [c[0] for c in eng.calls] == ["set_normalise", "infer_cutouts_mc_composite", "set_normalise"]
    assert eng.calls[1][3:] == (8, 9, 100)
    assert list(res.dtype.names) == ["list_idx", "shifts", "galaxy_distances_to_center_x", "galaxy_distances_to_center_y",
                                     "mse_center", "epistemic_norm", "passed_cuts"]
    assert res["epistemic_norm"].tolist() == [50.0, 100.0, 150.0] and res["passed_cuts"].tolist() == [True, True, False]
    res = db.deblend_field(dist, on_device=True, epistemic_criterion=60.0, mse_criterion=1e9)
    assert res["passed_cuts"].tolist() == [True, False, False]
    pred = db.get_predicted_field()
    assert (pred["predicted_epistemic_field"] == 3.0).all() and pred["predicted_epistemic_field"].shape == (F, F, NB)
    # without the estimate: the call, the columns and the zero epistemic field of before
    net = Net()
    db = DeblendField(net, fields, cutout_size=CS, nb_of_bands=NB)
    net._core.engine.infer_cutouts_composite = lambda field, starts, places, seed=0: (
        net._core.engine.calls.append(("infer_cutouts_composite", seed)) or
        {"mean_field": np.full(field.shape, 1.0), "stddev_field": np.full(field.shape, 2.0), "residual_field": field - 1.0,
         "mse_center": np.arange(len(starts), dtype=np.float64) * 60.0})
    res = db.deblend_field(dist, on_device=True)
    assert [c[0] for c in net._core.engine.calls] == ["set_normalise", "infer_cutouts_composite", "set_normalise"]
    assert "epistemic_norm" not in res.dtype.names and res["passed_cuts"].tolist() == [True, True, False]
    assert not db.get_predicted_field()["predicted_epistemic_field"].any()


def test_deblend_field_default_path_with_the_estimate_is_one_engine_call():
    from debvader_amd.deblend.field_deblender import DeblendField

    net, fields = Net(), _fields(1)
    db = DeblendField(net, fields, cutout_size=CS, nb_of_bands=NB, epistemic_uncertainty_estimation=True)
    dist = np.array([[0.0, 0.0], [5.0, -7.0], [-3.0, 11.0]])
    res = db.deblend_field(dist, mse_criterion=1e9, epistemic_criterion=120.0)
    eng = net._core.engine
    assert [c[0] for c in eng.calls] == ["set_normalise", "infer_cutouts_mc_keep", "set_normalise"]
    assert eng.calls[1][2:] == (8, 9, 100)                       # the seeds deblend() and deblend_epistemic() would draw
    assert list(res.dtype.names) == ["cutout_images", "output_images_mean", "output_images_stddev", "shifts", "list_idx",
                                     "galaxy_distances_to_center_x", "galaxy_distances_to_center_y", "epistemic_uncertainty",
                                     "passed_cuts"]
    assert res["epistemic_uncertainty"][1].dtype == np.float64 and (res["epistemic_uncertainty"][1] == 200.0).all()
    assert res["passed_cuts"].tolist() == [True, True, False]
