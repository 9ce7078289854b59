"""CPU checks of the many-field deblending path (DeblendFieldBatch, Engine.infer_fields*, Context.scene_fit_shifts_fields):
field_ptr validation, the split of per-field distance lists into one stamp list, fields without a valid galaxy, the
recarray columns of both modes, and the four C-ABI entry points.  The engine is a stand-in that records its calls, in the
manner of tests/stub_engine.py: no GPU is touched."""
import inspect

import numpy as np
import pytest

F, CS, NB = 81, 59, 6


class RecordingEngine:
    """Returns stamps that encode their global stamp number, and records every call."""

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


def test_field_ptr_validation():
    from debvader_amd.engine import check_field_ptr

    fp = check_field_ptr([0, 2, 2, 5], 3, 5)
    assert fp.dtype == np.int64 and fp.tolist() == [0, 2, 2, 5]
    assert check_field_ptr(np.array([0.0, 3.0]), 1, 3).tolist() == [0, 3]
    with pytest.raises(ValueError, match="one entry per field plus one"):
        check_field_ptr([0, 2, 5], 3, 5)
    with pytest.raises(ValueError, match="one entry per field plus one"):
        check_field_ptr([[0, 5]], 1, 5)
    with pytest.raises(ValueError, match="start at 0 and end at"):
        check_field_ptr([1, 2, 5], 2, 5)
    with pytest.raises(ValueError, match="start at 0 and end at"):
        check_field_ptr([0, 2, 4], 2, 5)
    with pytest.raises(ValueError, match="must not decrease"):
        check_field_ptr([0, 4, 3, 5], 3, 5)
    with pytest.raises(ValueError, match="integers"):
        check_field_ptr([0, 1.5, 5], 2, 5)


def test_public_calls_check_field_ptr_before_the_gpu():
    from debvader_amd import engine as E
    from debvader_amd.deblend_cutout.optimization import position_optimization_fields

    for name in ("infer_fields", "infer_fields_keep", "infer_fields_composite"):
        assert "field_ptr" in inspect.signature(getattr(E.Engine, name)).parameters
    assert "field_ptr" in inspect.signature(E.Context.scene_fit_shifts_fields).parameters
    params = list(inspect.signature(position_optimization_fields).parameters)
    assert params[:5] == ["field_images", "stamps", "distances", "field_ptr", "bound"]
    assert inspect.signature(position_optimization_fields).parameters["bound"].default == 3.0
    with pytest.raises(ValueError, match="field_ptr"):
        position_optimization_fields(np.zeros((2, 41, 41, 3)), np.zeros((3, 11, 11, 3)), np.zeros((3, 2)), [0, 1, 2])
    with pytest.raises(ValueError, match="band"):
        position_optimization_fields(np.zeros((2, 41, 41, 2)), np.zeros((3, 11, 11, 2)), np.zeros((3, 2)), [0, 1, 3])
    with pytest.raises(ValueError, match="square fields"):
        position_optimization_fields(np.zeros((41, 41, 3)), np.zeros((3, 11, 11, 3)), np.zeros((3, 2)), [0, 3])
    # the unbound methods validate before they touch self._h: a bare object stands in for the engine
    with pytest.raises(ValueError, match="field_ptr"):
        E.Engine.infer_fields(object(), np.zeros((2, F, F, NB)), [[0, 0]], [0, 2, 1])
    with pytest.raises(ValueError, match="square fields"):
        E.Engine.infer_fields_composite(object(), np.zeros((F, F, NB)), [[0, 0]], [[0, 0]], [0, 1])
    with pytest.raises(ValueError, match="placements"):
        E.Engine.infer_fields_composite(object(), np.zeros((1, F, F, NB)), [[0, 0]], [[0, 0], [1, 1]], [0, 1])
    with pytest.raises(ValueError, match="field_ptr"):
        E.Context.scene_fit_shifts_fields(object(), np.zeros((2, 41, 41)), np.zeros((3, 11, 11)), np.zeros((3, 2)), [0, 3])


def test_batch_windows_split():
    from debvader_amd.deblend.field_deblender import batch_windows
    from debvader_amd.extract.extraction import cutout_windows

    starts, fp, kept, dd = batch_windows(F, DIST, CS)
    assert fp.dtype == np.int64 and fp.tolist() == [0, 2, 2, 3, 3]
    assert [k.tolist() for k in kept] == [[0, 1], [], [1], []]
    assert starts.dtype == np.int32 and starts.shape == (3, 2)
    for m in (0, 2):
        st, ok = cutout_windows(F, DIST[m], CS)
        assert np.array_equal(starts[fp[m]:fp[m + 1]], st[ok])
    assert np.array_equal(dd, np.array([[0.0, 0.0], [5.0, -7.0], [-3.0, 11.0]]))
    # no field at all, and fields without any galaxy
    starts, fp, kept, dd = batch_windows(F, [], CS)
    assert starts.shape == (0, 2) and fp.tolist() == [0] and kept == [] and dd.shape == (0, 2)
    starts, fp, kept, dd = batch_windows(F, [np.array([]), []], CS)
    assert starts.shape == (0, 2) and fp.tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match="field 1"):
        batch_windows(F, [np.zeros((1, 2)), np.zeros((2, 3))], CS)


def test_on_device_pass_columns_places_and_empty_fields(capsys):
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch

    net, fields = Net(), _fields()
    db = DeblendFieldBatch(net, fields, cutout_size=CS, nb_of_bands=NB, normalise=True)
    res = db.deblend_fields(DIST, on_device=True)
    assert "too close from the border" in capsys.readouterr().out
    eng = net._core.engine
    assert [c[0] for c in eng.calls] == ["set_normalise", "infer_fields_composite", "set_normalise"]
    assert eng.calls[0][1] is True and eng.calls[2][1] is False
    _, starts, places, fp, seed = eng.calls[1]
    assert seed == 8 and fp.tolist() == [0, 2, 2, 3, 3]
    po = int((F - CS) / 2)
    assert np.array_equal(places, po + np.array([[0, 0], [5, -7], [-3, 11]]))
    assert np.array_equal(starts, places)                   # windows around the galaxies: integer distances
    assert res is db.res_deblend and len(res) == 4 and [len(r) for r in res] == [2, 0, 1, 0]
    want = [("list_idx", "int64"), ("shifts", "object"), ("galaxy_distances_to_center_x", "float64"),
            ("galaxy_distances_to_center_y", "float64"), ("mse_center", "float64"), ("passed_cuts", "bool")]
    for r in res:
        assert isinstance(r, np.recarray)
        assert [(k, str(r.dtype[k])) for k in r.dtype.names] == want
    assert res[0]["list_idx"].tolist() == [0, 1] and res[2]["list_idx"].tolist() == [1]
    assert res[2]["galaxy_distances_to_center_x"].tolist() == [-3.0]
    assert res[0]["mse_center"].tolist() == [0.0, 60.0] and res[2]["mse_center"].tolist() == [120.0]
    assert res[0]["passed_cuts"].tolist() == [True, True] and res[2]["passed_cuts"].tolist() == [False]
    assert all(np.array_equal(s, [0, 0]) for s in res[0]["shifts"])
    assert db.nb_of_detected_objects == [[2, 0, 2, 1]] and db.nb_of_deblended_galaxies == [[2, 0, 1, 0]]
    # the fields the engine composited come back as they are
    assert np.array_equal(db.get_residual_fields(), fields - 1.0)
    pred = db.get_predicted_fields()
    assert sorted(pred) == ["predicted_mean_fields", "predicted_stddev_fields"]
    assert pred["predicted_mean_fields"].shape == fields.shape and (pred["predicted_stddev_fields"] == 2.0).all()
    with pytest.raises(ValueError, match="output_images_mean"):
        db.optimise_positions()


def test_default_pass_columns_and_stamp_rows():
    from debvader_amd.deblend.field_deblender import DeblendField, DeblendFieldBatch

    net, fields = Net(), _fields()
    db = DeblendFieldBatch(net, fields, cutout_size=CS, nb_of_bands=NB)
    res = db.deblend_fields(DIST, mse_criterion=1.0e9)
    eng = net._core.engine
    assert [c[0] for c in eng.calls] == ["set_normalise", "infer_fields_keep", "set_normalise"]
    assert eng.calls[0][1] is False
    want = [("cutout_images", "object"), ("output_images_mean", "object"), ("output_images_stddev", "object"),
            ("shifts", "object"), ("list_idx", "int64"), ("galaxy_distances_to_center_x", "float64"),
            ("galaxy_distances_to_center_y", "float64"), ("epistemic_uncertainty", "object"), ("passed_cuts", "bool")]
    assert [len(r) for r in res] == [2, 0, 1, 0]
    for r in res:
        assert [(k, str(r.dtype[k])) for k in r.dtype.names] == want
    # the same column names, in the same order, as DeblendField's default recarray
    src = inspect.getsource(DeblendField.deblend_field)
    order = [src.index(f'res_deblend["{k}"] = ') for k, _ in want]
    assert order == sorted(order)
    # field 2's only row is global stamp 2, cut from field 2
    row = res[2][0]
    assert (row["output_images_mean"] == 2.0).all() and (row["output_images_stddev"] == 2.5).all()
    po = int((F - CS) / 2)
    assert np.array_equal(row["cutout_images"], fields[2, po - 3:po - 3 + CS, po + 11:po + 11 + CS])
    assert row["cutout_images"].dtype == np.float64 and row["output_images_mean"].dtype == np.float32
    assert row["epistemic_uncertainty"].shape == (CS, CS, NB) and not row["epistemic_uncertainty"].any()
    assert all(bool(p) for r in res for p in r["passed_cuts"])


def test_no_valid_galaxy_anywhere_is_not_an_error():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch

    for on_device in (False, True):
        net = Net()
        db = DeblendFieldBatch(net, _fields(2), cutout_size=CS, nb_of_bands=NB)
        res = db.deblend_fields([np.zeros((0, 2)), np.array([[70.0, 0.0]])], on_device=on_device)
        assert [len(r) for r in res] == [0, 0]
        call = net._core.engine.calls[1]
        assert call[1].shape == (0, 2) and call[-2].tolist() == [0, 0, 0]


def test_refusals_before_the_engine():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch

    net = Net()
    with pytest.raises(ValueError, match="expected fields"):
        DeblendFieldBatch(net, np.zeros((F, F, NB)), cutout_size=CS, nb_of_bands=NB)
    with pytest.raises(TypeError):
        DeblendFieldBatch(net, _fields(1), epistemic_uncertainty_estimation=True)
    db = DeblendFieldBatch(net, _fields(2), cutout_size=CS, nb_of_bands=NB)
    with pytest.raises(ValueError, match="2 fields but 1"):
        db.deblend_fields([np.zeros((0, 2))])
    with pytest.raises(ValueError, match="integer positions"):
        db.deblend_fields([np.array([[0.5, 0.0]]), np.zeros((0, 2))], on_device=True)
    assert net._core.engine.calls == []
    with pytest.raises(ValueError, match="no deblend_fields"):
        db.get_residual_fields()
    with pytest.raises(ValueError, match="runs on the engine"):
        DeblendFieldBatch(object(), _fields(1), cutout_size=CS, nb_of_bands=NB).deblend_fields([np.zeros((0, 2))])


def test_class_is_not_a_root_name():
    import debvader_amd

    assert not hasattr(debvader_amd, "DeblendFieldBatch")


def test_entry_points_are_bound():
    from debvader_amd import _lib

    for name in ("dv_infer_fields", "dv_infer_fields_keep", "dv_infer_fields_composite", "dv_scene_fit_shifts_fields"):
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.lib, name)
