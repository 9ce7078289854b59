"""CPU checks of the iterative loop's catalogue (IterativeDeblendFieldBatch.iterative_catalogue, DESIGN.md section
7m): the C ABI of the two new field-set calls, the numpy restatement of the end-of-loop sums on a case with a known answer,
and the host loop against a scripted stand-in for the set - the dtype of the records, the join of every pass's rows with the
end-of-loop sums by the resident row number across fields that stop at different passes, seen_before on hand-placed
centroids, the refusals, and the calls that are and are not made.  No GPU is touched."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import blend_oracle as bo
from tests import blend_set_oracle as bso
from tests.test_iterative_batch_host import CS, F, NB, ROOT, Core, ScriptedSet, StubEngine

NEW_SYMBOLS = ["dv_field_set_pass_measure", "dv_field_set_blend"]


def test_header_binding_export_map_and_library_have_the_new_symbols():
    from debvader_amd import _lib

    header = open(os.path.join(ROOT, "include", "debvader_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(dv_field_set\* set," % name, header), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    exports = open(os.path.join(ROOT, "debvader_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*dv_\*;", exports)
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW_SYMBOLS:
        assert re.search(r"\bT %s$" % name, dyn, re.M), name
    # the library refuses a null handle itself, without a GPU
    assert _lib.lib.dv_field_set_blend(None, 2, 0, None) == -1
    assert _lib.lib.dv_field_set_pass_measure(None, None, None, None, 0, 0, None, None, None, None, None, None, None, None,
                                              None, None) == -1


def test_restatement_on_a_galaxy_alone_in_its_field():
    """The field IS the galaxy's stamp at its placement, so the final residual is zero under the footprint: R1 = R2 = 0,
    and Bm = Bd = the child sum A of tests/blend_oracle.py."""
    cs, Fq, nb = 15, 40, 3
    yy, xx = np.mgrid[:cs, :cs]
    stamp = np.zeros((1, cs, cs, nb), np.float32)
    stamp[0, :, :, 2] = 3.0 * np.exp(-0.5 * ((yy - 7.3) ** 2 / 4.0 + (xx - 6.8) ** 2 / 5.0))
    shape, status = np.array([[7.3, 6.8, 4.0, 0.3, 5.0]]), np.array([0])
    for place in ((12, 9), (-4, 30)):                          # inside, and clipped at two edges
        places, fp = np.array([place]), np.array([0, 1])
        mean = bo.composite(stamp, places, fp, 1, Fq)
        base = mean.copy()
        final = base - mean
        got = bso.sums(cs, shape, status, places, [0], mean, base, final)
        child = bo.blend(stamp, shape, status, places, mean, base, fp)
        assert got["sums"][0, 2] == 0.0 and got["sums"][0, 3] == 0.0
        assert got["sums"][0, 0] == got["sums"][0, 1] == child["blend"][0, 1] > 0
        assert np.array_equal(got["sums"][0, :2], child["blend"][0, 2:])
    # a residual of one everywhere: R1 = R2 = W; no base: Bd NaN; a failed row: four NaN; a stamp off the field: zeros
    ones = np.ones_like(mean)
    got = bso.sums(cs, np.repeat(shape, 3, axis=0), [0, 3, 2], [(12, 9), (12, 9), (-cs, 0)], [0, 0, 0], mean, None, ones)
    W = bo.blend(stamp, shape, status, [(12, 9)], mean)["blend"][0, 0]
    assert got["sums"][0, 2] == got["sums"][0, 3] == W and np.isnan(got["sums"][0, 1])
    assert np.isnan(got["sums"][1]).all()
    assert got["sums"][2, 0] == got["sums"][2, 2] == got["sums"][2, 3] == 0.0 and np.isnan(got["sums"][2, 1])


# ---- the host loop against a scripted set ---------------------------------------------------------------------------------
class MeasuringSet(ScriptedSet):
    """ScriptedSet plus the two calls of section 7m.  A stamp's row is scripted by (pass, global stamp number of the pass):
    owner.rows[(k, i)] = (row, col, status), default (29, 29, 0).  Every value it returns encodes the stamp's resident row
    number r (stamps of all measured passes in call order), so that a wrong join shows: W = 10 + r, A = (r + 1) / 2,
    npix = r, and blend_sums row r = {r + .25, r + .5, r + .75, r + 1}."""

    def __init__(self, *a):
        super().__init__(*a)
        self.rows = 0

    def deblend_pass_measure(self, starts, places, field_ptr, seed=0, band=2, sigma0=3.0, tol=1e-10, max_iter=200, blend=True):
        k = self.k
        out = self.deblend_pass(starts, places, field_ptr, seed=seed)
        n = len(starts)
        self.owner.calls.append(("measure", dict(band=band, sigma0=sigma0, tol=tol, max_iter=max_iter, blend=blend)))
        r = self.rows + np.arange(n)
        shape = np.zeros((n, 5))
        status = np.zeros(n, np.int32)
        for i in range(n):
            row, col, st = self.owner.rows.get((k, i), (29.0, 29.0, 0))
            shape[i] = (row, col, 4.0 + i, 0.5, 6.0) if st != 3 else np.nan
            status[i] = st
        out.update(flux=np.outer(r + 1.0, np.arange(1, NB + 1)), flux_err=np.full((n, NB), 0.5), shape=shape,
                   iters=np.full(n, 7 + k, np.int32), status=status)
        if blend:
            npix = r.astype(np.int32)
            npix[status == 3] = -1
            out.update(child=np.stack([10.0 + r, (r + 1) / 2.0], axis=1), npix=npix)
            self.rows += n
        return out

    def blend_sums(self, band=2):
        assert not self.closed
        self.owner.calls.append(("sums", band))
        r = np.arange(self.rows, dtype=np.float64)
        return np.stack([r + 0.25, r + 0.5, r + 0.75, r + 1.0], axis=1)


class MeasuringEngine(StubEngine):
    def __init__(self, script, rows):
        super().__init__(script)
        self.rows = rows

    def open_field_set(self, fields, cumulative=False):
        self.calls.append(("open", bool(cumulative)))
        self.sets.append(MeasuringSet(self, np.asarray(fields), cumulative))
        return self.sets[-1]


class Net:
    def __init__(self, script, rows=None):
        self._core = Core(script)
        if rows is not None:
            self._core.engine = MeasuringEngine(script, rows)


def _run(script, rows=None, **kw):
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch

    net = Net(script, rows)
    fields = np.random.default_rng(1).normal(size=(len(script), F, F, NB))
    obj = IterativeDeblendFieldBatch(net, fields, CS, NB)
    return obj, (obj.iterative_catalogue(**kw) if kw else obj.iterative_deblending()), net._core


# field 0: 3 then 4 stamps, then nothing; field 1: 2; field 2: none; field 3: 1, 2, 3.  Per pass the stamps are numbered
# over the active fields: pass 0 = rows 0 .. 5 (f0: 0-2, f1: 3-4, f3: 5), pass 1 = 6 .. 11 (f0: 6-9, f3: 10-11), pass 2 =
# 12 .. 14 (f3)
SCRIPT = [[(3, 0), (4, 0)], [(2, 0)], [(0, 0)], [(1, 0), (2, 0), (3, 0)]]
RESIDENT = [[0, 1, 2, 6, 7, 8, 9], [3, 4], [], [5, 10, 11, 12, 13, 14]]
# Stamp i of a field is placed at p0 + (-i, +i).  Field 0, pass 1 (stamps 0 .. 3 of that pass), against its pass-0 rows
# at p0 + 29 + {(0, 0), (-1, 1), (-2, 2)}:
#   stamp 0 at (29, 29): on top of row 0                                     -> 0 (a match)
#   stamp 1 at (29.5, 28.5): p0 + 29 + (-.5, .5), sqrt(.5) from rows 0 and 1    -> 0 (a tie goes to the lowest index)
#   stamp 2 at (39, 29): ten pixels from everything                          -> -1 (a miss)
#   stamp 3 failed (status 3, NaN moments): the stamp centre p0 + 29 + (-3, 3), sqrt(2) from row 2 -> 2
ROWS = {(1, 1): (29.5, 28.5, 0), (1, 2): (39.0, 29.0, 0), (1, 3): (np.nan, np.nan, 3)}
SEEN = [[-1, -1, -1, 0, 0, -1, 2], [-1, -1], [], None]


def test_records_join_and_seen_before():
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch as B
    from debvader_amd.measure.measurement import blend_dtype, catalogue_dtype, residual_dtype

    obj, res, core = _run(SCRIPT, ROWS, measure=True, blendedness=True, band=1, sigma0=2.5, tol=1e-8, max_iter=50)
    assert [len(m) for m in obj.mse] == [2, 1, 0, 3]
    want = np.dtype(B.COLUMNS + catalogue_dtype(NB) + [("seen_before", "<i8")] + blend_dtype() + residual_dtype())
    for m, rec in enumerate(res):
        assert rec.dtype == want and isinstance(rec, np.recarray), m
        r = np.array(RESIDENT[m], dtype=np.float64)
        assert len(rec) == len(r), m
        # what every pass measured, row by row
        assert np.array_equal(rec["flux"], np.outer(r + 1.0, np.arange(1, NB + 1)))
        assert np.array_equal(rec["iters"], 7 + rec["iteration"])
        # ... and the end-of-loop sums, joined by the resident row number
        ok = rec["status"] != 3
        assert np.array_equal(rec["blend_weight"], 10.0 + r) and np.array_equal(rec["blend_child"], (r + 1) / 2.0)
        assert np.array_equal(rec["blend_npix"], np.where(ok, r, -1))
        assert np.array_equal(rec["blend_model"], r + 0.25) and np.array_equal(rec["blend_data"], r + 0.5)
        assert np.array_equal(rec["resid_sum"], r + 0.75) and np.array_equal(rec["resid_sq"], r + 1.0)
        assert np.array_equal(rec["blendedness"][ok], (1.0 - (r + 1) / 2.0 / (r + 0.25))[ok])
        assert np.array_equal(rec["blendedness_data"][ok], (1.0 - (r + 1) / 2.0 / (r + 0.5))[ok])
        assert np.array_equal(rec["resid_mean"][ok], ((r + 0.75) / (10.0 + r))[ok])
        assert np.array_equal(rec["resid_rms"][ok], np.sqrt((r + 1.0) / (10.0 + r))[ok])
        for k in ("blendedness", "blendedness_data", "resid_mean", "resid_rms", "sigma", "e1", "e2"):
            assert np.isnan(rec[k][~ok]).all(), k
        if SEEN[m] is not None:
            assert rec["seen_before"].tolist() == SEEN[m], m
    assert (res[0]["status"] == 3).sum() == 1 and res[0]["iteration"].tolist() == [0, 0, 0, 1, 1, 1, 1]
    # field 3: stamp i of every pass stands at p0 + 29 + (-i, i), sqrt(2) from stamp i - 1: a row sees its own stamp in the
    # earliest pass that has it (distance 0; among equals the lowest index), else the neighbouring stamp of an earlier pass
    assert res[3]["iteration"].tolist() == [0, 1, 1, 2, 2, 2] and res[3]["seen_before"].tolist() == [-1, 0, 0, 0, 2, 2]
    # the calls: every pass measured with the caller's parameters, one sums call after the last pass and before the reads
    names = [c[0] for c in core.engine.calls]
    assert names.count("measure") == names.count("pass") == 3 and names.count("sums") == 1
    assert all(c[1] == dict(band=1, sigma0=2.5, tol=1e-8, max_iter=50, blend=True) for c in core.engine.calls if c[0] == "measure")
    assert [c for c in core.engine.calls if c[0] == "sums"] == [("sums", 1)]
    tail = names[names.index("sums"):]
    assert tail == ["sums", "read", "read", "read", "close"] and "pass" not in tail
    assert core.seed_counter == 7 + 3


def test_seen_before_on_hand_placed_centroids():
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch as B

    it = np.array([0, 0, 1, 1, 1, 2, 2, 0])
    c = np.array([[10.0, 10.0], [10.0, 13.0], [10.0, 11.5], [11.0, 10.0], [50.0, 50.0], [10.0, 11.5], [np.nan, 3.0],
                  [10.0, 12.0]])
    # row 2: 1.5 from rows 0 and 1, 0.5 from row 7 (pass 0, a later index): the nearest; row 3: 1 from row 0; row 4: a
    # miss; row 5: on top of row 2 (pass 1); row 6: a NaN centroid matches nothing; pass-0 rows: -1
    assert B.seen_before(it, c, 2.0).tolist() == [-1, -1, 7, 0, -1, 2, -1, -1]
    assert B.seen_before(it, c, 0.4).tolist() == [-1, -1, -1, -1, -1, 2, -1, -1]
    # exactly on the radius counts; a tie goes to the lowest index
    assert B.seen_before([0, 0, 1], [[0.0, 2.0], [2.0, 0.0], [0.0, 0.0]], 2.0).tolist() == [-1, -1, 0]
    assert B.seen_before([], np.zeros((0, 2)), 2.0).tolist() == []


def test_measure_without_blendedness_and_the_shared_columns():
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch as B
    from debvader_amd.measure.measurement import catalogue_dtype

    plain_obj, plain, plain_core = _run(SCRIPT)
    obj, res, core = _run(SCRIPT, ROWS, measure=True)
    assert "sums" not in [c[0] for c in core.engine.calls]
    assert all(c[1]["blend"] is False for c in core.engine.calls if c[0] == "measure")
    assert obj.mse == plain_obj.mse and core.seed_counter == plain_core.seed_counter
    for rec, p in zip(res, plain):
        assert rec.dtype == np.dtype(B.COLUMNS + catalogue_dtype(NB) + [("seen_before", "<i8")])
        assert p.dtype == np.dtype(B.COLUMNS)
        for k in p.dtype.names:
            if k == "shifts":
                assert all(np.array_equal(a, b) for a, b in zip(rec[k], p[k]))
            else:
                assert np.array_equal(rec[k], p[k]), k
    assert res[0]["seen_before"].tolist() == SEEN[0]


def test_measure_false_makes_the_four_old_calls_only():
    # the set of tests/test_iterative_batch_host.py has detect, deblend_pass, read and close and nothing else
    obj, res, core = _run(SCRIPT)
    assert type(core.engine.sets[0]) is ScriptedSet
    assert not hasattr(ScriptedSet, "deblend_pass_measure") and not hasattr(ScriptedSet, "blend_sums")
    assert {c[0] for c in core.engine.calls} == {"open", "set_normalise", "detect", "pass", "read", "close"}
    assert [len(r) for r in res] == [7, 2, 0, 6]


def test_return_fields_false_reads_nothing():
    obj, res, core = _run(SCRIPT, ROWS, measure=True, blendedness=True, return_fields=False)
    names = [c[0] for c in core.engine.calls]
    assert "read" not in names and names[-2:] == ["sums", "close"]
    for getter in (obj.get_residual_fields, obj.get_predicted_fields):
        with pytest.raises(ValueError, match="return_fields"):
            getter()
    full = _run(SCRIPT, ROWS, measure=True, blendedness=True)[1]
    for a, b in zip(res, full):
        for k in a.dtype.names:
            if k != "shifts":
                assert np.array_equal(a[k], b[k], equal_nan=a.dtype[k].kind == "f"), k
    # the plain loop without fields, and a later run with them on the same object
    obj2, _, core2 = _run(SCRIPT, return_fields=False)
    assert "read" not in [c[0] for c in core2.engine.calls]
    with pytest.raises(ValueError, match="return_fields"):
        obj2.get_residual_fields()
    obj2.iterative_deblending()
    assert obj2.get_residual_fields().shape == (4, F, F, NB)


def test_refusals():
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch

    with pytest.raises(ValueError, match="measure=True"):
        _run(SCRIPT, ROWS, blendedness=True)
    with pytest.raises(ValueError, match="match_radius"):
        _run(SCRIPT, ROWS, measure=True, match_radius=-1.0)
    net = Net(SCRIPT, ROWS)
    obj = IterativeDeblendFieldBatch(net, np.zeros((4, F, F, NB)), CS, NB)
    with pytest.raises(ValueError, match="no iterative_deblending"):
        obj.get_residual_fields()
    with pytest.raises(ValueError, match="measure=True"):
        obj.iterative_catalogue(blendedness=True)
    assert net._core.engine.calls == []                       # refused before the set is opened


def test_residual_column_helpers():
    from debvader_amd.measure.measurement import residual_dtype, residual_records

    assert [n for n, _ in residual_dtype()] == ["resid_sum", "resid_sq", "resid_mean", "resid_rms"]
    W = np.array([2.0, 4.0, 0.0, -1.0, np.nan, 3.0])
    npix = np.array([5, 9, 0, 4, 4, -1])
    R1, R2 = np.array([1.0, -2.0, 0.0, 1.0, 1.0, np.nan]), np.array([8.0, 1.0, 0.0, 1.0, 1.0, np.nan])
    rec = residual_records(W, npix, R1, R2)
    assert np.array_equal(rec["resid_sum"], R1, equal_nan=True) and np.array_equal(rec["resid_sq"], R2, equal_nan=True)
    assert rec["resid_mean"][:2].tolist() == [0.5, -0.5] and rec["resid_rms"][:2].tolist() == [2.0, 0.5]
    assert np.isnan(rec["resid_mean"][2:]).all() and np.isnan(rec["resid_rms"][2:]).all()
    assert len(residual_records([], [], [], [])) == 0
