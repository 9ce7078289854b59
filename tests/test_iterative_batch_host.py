"""CPU checks of the many-field iterative deblender (IterativeDeblendFieldBatch): the C ABI of the
resident field set, and the host loop run against a stand-in for the set that returns scripted catalogues - the stopping
rules of both modes, the shrinking active mask, the list_idx offsets and the iteration column, the seeds, the empty-pass
departure from IterativeDeblendField and the refusals.  No GPU is touched."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, CS, NB = 81, 59, 6          # a window fits when the distance to the centre is within +-11 on both axes
SET_SYMBOLS = ["dv_field_set_open", "dv_field_set_detect", "dv_field_set_pass", "dv_field_set_read", "dv_field_set_close"]


def test_header_declares_the_field_set_and_the_export_map_covers_it():
    from debvader_amd import _lib

    header = open(os.path.join(ROOT, "include", "debvader_hip.h")).read()
    for name in SET_SYMBOLS:
        assert re.search(r"\bint %s\(dv_" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert "typedef struct dv_field_set dv_field_set;" in header
    for which in ("WORK", "FINAL", "MEAN", "STDDEV"):
        assert "#define DV_FIELD_SET_" + which in header
    # the version script exports the dv_ prefix and nothing else: the new names need no entry of their own
    exports = open(os.path.join(ROOT, "debvader_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*dv_\*;", exports) and re.search(r"local:\s*\*;", exports)
    # open / close on a null handle are refused by the library itself, without a GPU
    assert _lib.lib.dv_field_set_close(None) == -1 and _lib.lib.dv_field_set_read(None, 0, None) == -1


class ScriptedSet:
    """Stands in for engine.FieldSet: script[m][k] = (valid, invalid) detections of field m in its pass k."""

    def __init__(self, owner, fields, cumulative):
        self.owner, self.M, self.cumulative, self.k, self.closed = owner, len(fields), cumulative, 0, False
        self.fields = fields

    def detect(self, active=None):
        assert not self.closed
        active = np.ones(self.M, bool) if active is None else np.array(active, dtype=bool)
        self.owner.calls.append(("detect", active.copy()))
        xs, ys, off = [], [], [0]
        for m in range(self.M):
            script = self.owner.script[m]
            valid, invalid = script[self.k] if active[m] and self.k < len(script) else (0, 0)
            for i in range(valid):                       # distances (row, col) = (3 - i, i - 3) + 10 * pass
                xs.append(40.0 + (i - 3) + 0.2)
                ys.append(40.0 + (3 - i) - 0.3)
            for i in range(invalid):
                xs.append(2.0 + i)
                ys.append(40.0)
            off.append(len(xs))
        return {"x": np.array(xs), "y": np.array(ys), "offsets": np.array(off, np.int64)}

    def deblend_pass(self, starts, places, field_ptr, seed=0):
        assert not self.closed
        self.owner.calls.append(("pass", np.array(starts), np.array(places), np.array(field_ptr), seed))
        self.k += 1
        n = len(starts)
        field_mse = np.full(self.M, np.nan)
        has = np.diff(field_ptr) > 0
        field_mse[has] = 100.0 * self.k + np.arange(self.M)[has]
        return {"mse_center": np.arange(n, dtype=np.float64) * 30.0, "field_mse": field_mse}

    def read(self, which):
        assert not self.closed
        self.owner.calls.append(("read", which))
        return np.full(self.fields.shape, {"final": 1.0, "mean": 2.0, "stddev": 3.0}[which])

    def close(self):
        self.closed = True
        self.owner.calls.append(("close",))


class StubEngine:
    def __init__(self, script):
        self.script, self.calls, self.sets = script, [], []

    def set_normalise(self, on):
        self.calls.append(("set_normalise", bool(on)))

    def open_field_set(self, fields, cumulative=False):
        self.calls.append(("open", bool(cumulative)))
        self.sets.append(ScriptedSet(self, np.asarray(fields), cumulative))
        return self.sets[-1]


class Core:
    def __init__(self, script):
        self.engine, self.ctx, self.seed_counter = StubEngine(script), None, 7

    def next_seed(self):
        self.seed_counter += 1
        return self.seed_counter


class Net:
    def __init__(self, script):
        self._core = Core(script)


def _run(script, mode="reference", **kw):
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch

    net = Net(script)
    fields = np.random.default_rng(1).normal(size=(len(script), F, F, NB))
    obj = IterativeDeblendFieldBatch(net, fields, CS, NB)
    res = obj.iterative_deblending(mode=mode, **kw)
    return obj, res, net._core


def _calls(core, name):
    return [c for c in core.engine.calls if c[0] == name]


def test_package_exports_and_signatures():
    import debvader_amd
    from debvader_amd import deblend_iterative
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch
    from debvader_amd.deblend_iterative.iterative_deblender import IterativeDeblendField, IterativeDeblendFieldBatch

    assert deblend_iterative.IterativeDeblendFieldBatch is IterativeDeblendFieldBatch
    assert deblend_iterative.IterativeDeblendField is IterativeDeblendField
    assert "IterativeDeblendFieldBatch" not in dir(debvader_amd) and not hasattr(debvader_amd, "IterativeDeblendFieldBatch")
    assert list(inspect.signature(IterativeDeblendFieldBatch.__init__).parameters) == [
        "self", "net", "field_images", "cutout_size", "nb_of_bands", "normalise"]
    sig = inspect.signature(IterativeDeblendFieldBatch.iterative_deblending)
    assert list(sig.parameters) == ["self", "mse_criterion", "mode", "max_iterations"]
    assert sig.parameters["mode"].default == "reference" and sig.parameters["max_iterations"].default is None
    assert IterativeDeblendFieldBatch.COLUMNS == DeblendFieldBatch.ON_DEVICE_COLUMNS + [("iteration", "<i8")]


def test_reference_stopping_rule_and_shrinking_active_mask():
    # field 0: 5, 7, 7 -> three passes; field 1: 5, 3 -> two; field 2: nothing -> none; field 3: 2, 4, 6, 1 -> four
    script = [[(5, 0), (7, 0), (7, 0), (7, 0)], [(5, 0), (3, 0), (9, 0)], [(0, 0)], [(2, 0), (4, 1), (6, 0), (1, 0), (5, 0)]]
    obj, res, core = _run(script)
    assert [len(m) for m in obj.mse] == [3, 2, 0, 4]
    assert [len(r) for r in res] == [19, 8, 0, 13]
    masks = [c[1].tolist() for c in _calls(core, "detect")]
    assert masks == [[True, True, True, True], [True, True, False, True], [True, False, False, True],
                     [False, False, False, True]]
    assert obj.nb_of_deblended_galaxies == [[5, 5, 0, 2], [7, 3, 0, 4], [7, 0, 0, 6], [0, 0, 0, 1]]
    assert obj.nb_of_detected_objects == [[5, 5, 0, 2], [7, 3, 0, 5], [7, 0, 0, 6], [0, 0, 0, 1]]
    # stamps are numbered over the active fields, field after field
    fps = [c[3].tolist() for c in _calls(core, "pass")]
    assert fps == [[0, 5, 10, 10, 12], [0, 7, 10, 10, 14], [0, 7, 7, 7, 13], [0, 0, 0, 0, 1]]
    # the set is opened once in reference mode, read at the end and closed
    assert _calls(core, "open") == [("open", False)]
    assert [c[1] for c in _calls(core, "read")] == ["final", "mean", "stddev"] and core.engine.calls[-1] == ("close",)
    assert obj.get_residual_fields().shape == (4, F, F, NB) and (obj.get_residual_fields() == 1.0).all()
    pred = obj.get_predicted_fields()
    assert sorted(pred) == ["predicted_mean_fields", "predicted_stddev_fields"]
    assert (pred["predicted_mean_fields"] == 2.0).all() and (pred["predicted_stddev_fields"] == 3.0).all()
    # mse: the set's field_mse of every pass a field took
    assert obj.mse[0] == [100.0, 200.0, 300.0] and obj.mse[1] == [101.0, 201.0] and obj.mse[3] == [103.0, 203.0, 303.0, 403.0]


def test_records_list_idx_offsets_iteration_and_cuts():
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch

    script = [[(2, 0), (4, 1), (4, 0)], [(1, 0), (1, 0)]]
    obj, res, core = _run(script, mse_criterion=100.0)
    r0 = res[0]
    assert r0.dtype == np.dtype(IterativeDeblendFieldBatch.COLUMNS) and isinstance(r0, np.recarray)
    assert r0["iteration"].tolist() == [0, 0, 1, 1, 1, 1, 2, 2, 2, 2]
    # list_idx: the index in the pass's catalogue plus the galaxies deblended in earlier passes (the reference's offset)
    assert r0["list_idx"].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]
    assert res[1]["list_idx"].tolist() == [0, 1] and res[1]["iteration"].tolist() == [0, 1]
    # distances: detection._distances of the catalogue (rounded), places = int((F - cs) / 2) + distance
    assert r0["galaxy_distances_to_center_x"][:2].tolist() == [3.0, 2.0]
    assert r0["galaxy_distances_to_center_y"][:2].tolist() == [-3.0, -2.0]
    first = _calls(core, "pass")[0]
    assert first[1].tolist() == [[14, 8], [13, 9], [14, 8]] and first[2].tolist() == [[14, 8], [13, 9], [14, 8]]
    assert first[1].dtype.kind == "i" and first[2].dtype.kind == "i"
    # mse_center rows are the call's global rows; passed_cuts = ~(mse_center > criterion)
    assert r0["mse_center"][:2].tolist() == [0.0, 30.0] and res[1]["mse_center"][0] == 60.0
    second = r0[r0["iteration"] == 1]
    assert second["mse_center"].tolist() == [0.0, 30.0, 60.0, 90.0]
    third = r0[r0["iteration"] == 2]
    assert third["mse_center"].tolist() == [0.0, 30.0, 60.0, 90.0]
    obj2, res2, _ = _run([[(6, 0)]], mse_criterion=100.0)
    assert res2[0]["mse_center"].tolist() == [0.0, 30.0, 60.0, 90.0, 120.0, 150.0]
    assert res2[0]["passed_cuts"].tolist() == [True, True, True, True, False, False]
    assert all(np.array_equal(s, [0, 0]) for s in r0["shifts"])


def test_invalid_windows_are_dropped_and_offsets_count_deblended_galaxies():
    # pass 1 of the field: five detections, the first four fit -> list_idx 0..3 offset by the 2 of pass 0
    script = [[(2, 0), (4, 1)]]
    obj, res, core = _run(script)
    assert res[0]["list_idx"].tolist() == [0, 1, 2, 3, 4, 5]
    assert obj.nb_of_detected_objects == [[2], [5]] and obj.nb_of_deblended_galaxies == [[2], [4]]


def test_one_seed_per_pass_that_has_stamps():
    script = [[(5, 0), (7, 0), (7, 0)], [(5, 0), (3, 0)]]
    obj, res, core = _run(script)
    assert [c[4] for c in _calls(core, "pass")] == [8, 9, 10] and core.seed_counter == 10
    # normalise is set around every pass and cleared again
    norm = [c[1] for c in _calls(core, "set_normalise")]
    assert norm == [False, False] * 3
    # a last pass without any stamp draws no seed and makes no network call
    obj, res, core = _run([[(3, 0), (5, 0), (0, 2)]])
    assert len(_calls(core, "detect")) == 3 and len(_calls(core, "pass")) == 2 and core.seed_counter == 9
    # nothing at all: no call, no seed
    obj, res, core = _run([[(0, 0)], [(0, 3)]])
    assert len(_calls(core, "detect")) == 1 and not _calls(core, "pass") and core.seed_counter == 7
    assert obj.mse == [[], []] and [len(r) for r in res] == [0, 0]
    assert obj.nb_of_detected_objects == [] and obj.nb_of_deblended_galaxies == []


def test_empty_pass_contributes_nothing():
    """The departure from IterativeDeblendField: that class returns its previous recarray for an empty pass, and its loop
    appends it a second time with an mse of 0."""
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch

    # field 0: 3, 5, then a pass with detections that do not fit; field 1 goes on beside it
    script = [[(3, 0), (5, 0), (0, 2), (9, 0)], [(1, 0), (2, 0), (3, 0), (3, 0)]]
    obj, res, core = _run(script)
    assert len(res[0]) == 8 and res[0]["list_idx"].tolist() == list(range(8))          # no duplicated tail
    assert res[0]["iteration"].tolist() == [0] * 3 + [1] * 5
    assert len(obj.mse[0]) == 2 and 0.0 not in obj.mse[0]
    assert len(obj.mse[1]) == 4
    masks = [c[1].tolist() for c in _calls(core, "detect")]
    assert masks == [[True, True], [True, True], [True, True], [False, True]]
    # a field whose first pass is empty: an empty recarray with the on-device columns, mse == []
    obj, res, core = _run([[(0, 0)], [(2, 0)]])
    assert len(res[0]) == 0 and res[0].dtype == np.dtype(IterativeDeblendFieldBatch.COLUMNS) and obj.mse[0] == []
    assert isinstance(res[0], np.recarray) and len(res[1]) == 2


def test_cumulative_rule_and_max_iterations():
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch

    # counts that would stop the reference's rule after two passes go on while a pass deblends anything
    script = [[(5, 0), (3, 0), (1, 0), (0, 0)], [(2, 0), (0, 1), (4, 0)]]
    obj, res, core = _run(script, mode="cumulative")
    assert _calls(core, "open") == [("open", True)]
    assert [len(m) for m in obj.mse] == [3, 1] and [len(r) for r in res] == [9, 2]
    assert [c[1].tolist() for c in _calls(core, "detect")] == [[True, True], [True, True], [True, False], [True, False]]
    obj, res, core = _run(script, mode="cumulative", max_iterations=2)
    assert [len(m) for m in obj.mse] == [2, 1] and len(_calls(core, "detect")) == 2
    # the finite default of the mode
    assert IterativeDeblendFieldBatch.DEFAULT_MAX_ITERATIONS_CUMULATIVE == 10
    assert "10" in IterativeDeblendFieldBatch.iterative_deblending.__doc__
    obj, res, core = _run([[(1, 0)] * 30], mode="cumulative")
    assert len(obj.mse[0]) == 10 and len(res[0]) == 10 and res[0]["iteration"].tolist() == list(range(10))
    # max_iterations also bounds the reference mode
    obj, res, core = _run([[(1, 0), (2, 0), (3, 0), (4, 0)]], max_iterations=3)
    assert len(obj.mse[0]) == 3
    obj, res, core = _run([[(1, 0)]], max_iterations=0)
    assert obj.mse == [[]] and len(res[0]) == 0 and not _calls(core, "detect")


def test_refusals_name_the_alternative():
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch

    fields = np.zeros((2, F, F, NB))
    with pytest.raises(ValueError, match="IterativeDeblendField"):
        IterativeDeblendFieldBatch(lambda x: x, fields, CS, NB)

    class NoEngine:
        class _core:
            engine = None

    with pytest.raises(ValueError, match="load_deblender"):
        IterativeDeblendFieldBatch(NoEngine(), fields, CS, NB)
    with pytest.raises(ValueError, match="band 2.*DeblendFieldBatch"):
        IterativeDeblendFieldBatch(Net([[]]), np.zeros((2, F, F, 2)), CS, 2)
    with pytest.raises(ValueError, match=r"\(M, F, F, 6\)"):
        IterativeDeblendFieldBatch(Net([[]]), np.zeros((F, F, NB)), CS, NB)
    obj = IterativeDeblendFieldBatch(Net([[(1, 0)]] * 2), fields, CS, NB)
    with pytest.raises(ValueError, match="'reference'.*'cumulative'"):
        obj.iterative_deblending(mode="additive")
    with pytest.raises(ValueError, match="max_iterations"):
        obj.iterative_deblending(max_iterations=-1)
    with pytest.raises(ValueError, match="no iterative_deblending"):
        obj.get_residual_fields()
    # the set is closed even when a pass fails
    net = Net([[(1, 0)]])
    net._core.engine.script = None
    obj = IterativeDeblendFieldBatch(net, fields[:1], CS, NB)
    with pytest.raises(TypeError):
        obj.iterative_deblending()
    assert net._core.engine.sets[0].closed


def test_field_set_binding_checks_before_the_library():
    """engine.FieldSet validates what the C ABI cannot: shapes, integer rows, the field_ptr."""
    from debvader_amd import engine as E

    assert E.FieldSet.WHICH == {"work": 0, "final": 1, "mean": 2, "stddev": 3}
    assert list(inspect.signature(E.Engine.open_field_set).parameters) == ["self", "fields", "cumulative"]
    assert list(inspect.signature(E.FieldSet.deblend_pass).parameters) == ["self", "starts", "places", "field_ptr", "seed"]
    fs = E.FieldSet.__new__(E.FieldSet)
    fs._h, fs.shape = None, (2, F, F, NB)
    with pytest.raises(E._lib.DvError, match="closed") as e:
        fs.read("work")
    assert e.value.status == -5
    with pytest.raises(E._lib.DvError, match="closed"):
        fs.detect()
    with pytest.raises(E._lib.DvError, match="closed"):
        fs.deblend_pass(np.zeros((0, 2)), np.zeros((0, 2)), [0, 0, 0])
    fs.close()                                           # idempotent
