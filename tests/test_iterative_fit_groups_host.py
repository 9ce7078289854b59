"""CPU checks of the grouped joint flux fit of the iterative loop (FieldSet.fit_flux_groups, dv_field_set_fit_flux_groups,
IterativeDeblendFieldBatch.iterative_catalogue(fit_flux=True, fit_groups=True)): the C ABI of the new
call; the host loop against a scripted stand-in for the set whose every value encodes its resident row number - which calls
are made and which are not, the order and dtypes of the columns, the join by resident row, fit_group as an index into the
field's own recarray, the refusals, the unchanged call list at the default; and the definition in the joint order on the numpy
restatement of section 7w (tests/fit_flux_groups_oracle.py) for a two-pass field stated by hand.  No GPU is touched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import fit_flux_groups_oracle as fgo
from tests import fit_flux_oracle as ffo
from tests.test_iterative_batch_host import CS, F, NB, ROOT, ScriptedSet
from tests.test_iterative_catalogue_host import RESIDENT, ROWS, SCRIPT, Net
from tests.test_iterative_fit_flux_host import CTYPES, FittingEngine, FittingSet, _fit_row, _flux, _regroup, _stack

NEW_SYMBOL = "dv_field_set_fit_flux_groups"
# the argument counts of the entry points that were there before
BEFORE = {"dv_field_set_fit_flux": 24, "dv_field_set_keep_stamps": 2, "dv_scene_fit_flux_groups": 21, "dv_scene_fit_groups": 16,
          "dv_field_set_blend": 4, "dv_field_set_pass_measure": 16}


@pytest.fixture(autouse=True)
def _the_grouped_joint_fit_exists():
    """Everything here pins section 7y, the restatement in the joint order included: it is the rule of a call that must exist"""
    import inspect

    from debvader_amd import _lib
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch
    from debvader_amd.engine import FieldSet

    assert NEW_SYMBOL in _lib.SIGNATURES and hasattr(FieldSet, "fit_flux_groups")
    assert "fit_groups" in inspect.signature(IterativeDeblendFieldBatch.iterative_catalogue).parameters


def test_header_binding_export_map_and_library_have_the_new_symbol():
    from debvader_amd import _lib

    ctypes_of = dict(CTYPES)
    ctypes_of["const dv_fit_flux_params*"] = C.POINTER(_lib.DvFitFluxParams)
    header = open(os.path.join(ROOT, "include", "debvader_hip.h")).read()
    decl = re.search(r"\bint %s\(([^;]*)\);" % NEW_SYMBOL, header)
    assert decl, NEW_SYMBOL
    args = [" ".join(a.split()[:-1]) for a in decl.group(1).replace("\n", " ").split(",")]
    names = [a.split()[-1] for a in decl.group(1).replace("\n", " ").split(",")]
    assert names == ["set", "n_expected", "data", "weight", "params", "fit_scale", "fit_var", "fit_gram", "fit_proj", "fit_status",
                     "fit_chi2", "fit_npix", "fit_group", "fit_group_size"]
    restype, argtypes = _lib.SIGNATURES[NEW_SYMBOL]
    assert restype is C.c_int and argtypes == [ctypes_of[a] for a in args]
    assert getattr(_lib.lib, NEW_SYMBOL).argtypes == argtypes
    for name, count in BEFORE.items():
        old = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert old and len(old.group(1).split(",")) == count == len(_lib.SIGNATURES[name][1]), name
    exports = open(os.path.join(ROOT, "debvader_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*dv_\*;", exports)
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT %s$" % NEW_SYMBOL, dyn, re.M)
    # the library refuses a null handle itself, without a GPU
    assert getattr(_lib.lib, NEW_SYMBOL)(None, 0, None, None, None, *[None] * 9) == -1


def test_the_method_checks_its_arguments_before_the_library_call():
    from debvader_amd.engine import FieldSet

    fs = FieldSet.__new__(FieldSet)
    fs._h, fs.shape, fs.cumulative, fs._rows = C.c_void_p(1), (2, F, F, NB), True, 0     # (never reaches the library)
    fs.close = lambda: None
    with pytest.raises(ValueError, match="cumulative set keeps no copy"):
        fs.fit_flux_groups()
    with pytest.raises(ValueError, match="expected data fields of the shape"):
        fs.fit_flux_groups(data_fields=np.zeros((1, F, F, NB)))
    D = np.zeros((2, F, F, NB))
    with pytest.raises(ValueError, match="shape of the data fields"):
        fs.fit_flux_groups(data_fields=D, weight_fields=np.ones((2, F, F, NB + 1)))
    with pytest.raises(ValueError, match="min_pivot"):
        fs.fit_flux_groups(data_fields=D, min_pivot=1.0)
    with pytest.raises(ValueError, match="scratch_bytes"):
        fs.fit_flux_groups(data_fields=D, scratch_bytes=0)
    fs._h = C.c_void_p()


# ---- the host loop against a scripted set ---------------------------------------------------------------------------------
def _group_of(r):
    """What the scripted grouped fit returns for resident row r: the rows of a field, in recarray order, fall into groups of three
    consecutive rows - the label is the index of the group's first row in the field's recarray, whatever its pass"""
    for rows in RESIDENT:
        if r in rows:
            k = rows.index(r)
            return 3 * (k // 3), min(3, len(rows) - 3 * (k // 3))
    raise AssertionError(r)


class GroupedSet(FittingSet):
    """FittingSet plus the call of section 7y"""

    def fit_flux_groups(self, data_fields=None, weight_fields=None, min_pivot=1e-8, scratch_bytes=256 << 20):
        assert not self.closed
        self.owner.calls.append(("fit_groups", dict(data=data_fields, weights=weight_fields, min_pivot=min_pivot)))
        rows = [_fit_row(r) for r in range(self.rows)]
        keys = ["fit_scale", "fit_var", "fit_gram", "fit_proj", "fit_status"]
        keys += ["fit_chi2", "fit_npix"] if weight_fields is not None else []
        out = {k: np.array([row[k] for row in rows]).reshape(self.rows, NB) for k in keys}
        g = np.array([_group_of(r) for r in range(self.rows)], np.int32).reshape(self.rows, 2)
        out["fit_group"], out["fit_group_size"] = g[:, 0].copy(), g[:, 1].copy()
        return out


class GroupedEngine(FittingEngine):
    def open_field_set(self, fields, cumulative=False):
        self.calls.append(("open", bool(cumulative)))
        self.sets.append(GroupedSet(self, np.asarray(fields), cumulative))
        return self.sets[-1]


def _run(engine=GroupedEngine, **kw):
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch

    net = Net(SCRIPT, ROWS)
    net._core.engine = engine(SCRIPT, ROWS)
    fields = np.random.default_rng(1).normal(size=(len(SCRIPT), F, F, NB))
    obj = IterativeDeblendFieldBatch(net, fields, CS, NB)
    return obj, obj.iterative_catalogue(**kw), net._core


def test_columns_join_calls_and_the_group_as_an_index_into_the_recarray():
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch as B
    from debvader_amd.measure import measurement as ms

    assert ms.fit_groups_dtype(NB) == [("fit_group", "<i4"), ("fit_group_size", "<i4")]
    obj, res, core = _run(measure=True, blendedness=True, fit_flux=True, fit_groups=True, min_pivot=1e-6)
    assert [len(m) for m in obj.mse] == [2, 1, 0, 3]
    want = np.dtype(B.COLUMNS + B.catalogue_columns(NB, True) + ms.fit_flux_dtype(NB) + ms.fit_groups_dtype(NB))
    for m, rec in enumerate(res):
        assert rec.dtype == want and isinstance(rec, np.recarray), m
        r = np.array(RESIDENT[m], dtype=np.int64)
        assert len(rec) == len(r)
        for k in ("fit_scale", "fit_var", "fit_gram", "fit_proj", "fit_status"):
            assert np.array_equal(rec[k], _stack(r, k)), (m, k)
        assert np.array_equal(rec["flux_fit"], _stack(r, "fit_scale") * _flux(r))
        assert np.array_equal(rec["blend_model"], r + 0.25)
        # the join by resident row, and the label as an index into THIS recarray: the row it names is its own group's first
        assert rec["fit_group"].tolist() == [_group_of(x)[0] for x in r] and rec["fit_group"].dtype == np.int32
        assert rec["fit_group_size"].tolist() == [_group_of(x)[1] for x in r]
        if len(rec):
            root = rec[rec["fit_group"]]
            assert np.array_equal(root["fit_group"], rec["fit_group"]) and (rec["fit_group"] <= np.arange(len(rec))).all()
            assert np.array_equal(np.bincount(rec["fit_group"], minlength=len(rec))[rec["fit_group"]], rec["fit_group_size"])
    # field 0: rows 0 - 2 of pass 0 and rows 3 - 6 of pass 1; the group of recarray row 3 holds rows of pass 1 only, the label
    # of row 6 is 6
    assert res[0]["fit_group"].tolist() == [0, 0, 0, 3, 3, 3, 6] and res[0]["iteration"].tolist() == [0, 0, 0, 1, 1, 1, 1]
    assert obj.sky_fit is None and obj.nonneg_fit is None
    # the calls: the switch once before the first pass, one grouped fit before the reads and the close, never the dense one
    calls = [x[0] for x in core.engine.calls]
    assert calls.count("keep") == 1 and calls.index("keep") == calls.index("open") + 1 < calls.index("detect")
    assert all(x[1]["blend"] is True for x in core.engine.calls if x[0] == "measure") and calls.count("measure") == 3
    assert calls.count("fit_groups") == 1 and "fit" not in calls and calls.count("sums") == 1
    assert calls[calls.index("sums"):] == ["sums", "fit_groups", "read", "read", "read", "close"]
    fit_call = [x for x in core.engine.calls if x[0] == "fit_groups"][0][1]
    assert fit_call == dict(data=None, weights=None, min_pivot=1e-6)          # reference mode: the resident base
    # without blendedness and without the field downloads
    _, res2, core2 = _run(measure=True, fit_flux=True, fit_groups=True, return_fields=False)
    calls = [x[0] for x in core2.engine.calls]
    assert calls[-2:] == ["fit_groups", "close"] and "read" not in calls and "sums" not in calls and "fit" not in calls
    assert res2[3].dtype == np.dtype(B.COLUMNS + B.catalogue_columns(NB, False) + ms.fit_flux_dtype(NB) + ms.fit_groups_dtype(NB))


def test_weighted_columns_and_the_fields_in_cumulative_mode():
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch as B
    from debvader_amd.measure import measurement as ms

    W = np.random.default_rng(2).uniform(0.5, 2.0, size=(4, F, F, NB))
    obj, res, core = _run(measure=True, fit_flux=True, fit_weights=W, fit_groups=True, mode="cumulative", max_iterations=3)
    want = np.dtype(B.COLUMNS + B.catalogue_columns(NB, False) + ms.fit_flux_dtype(NB)
                    + [("fit_chi2", "<f8", (NB,)), ("fit_npix", "<i4", (NB,))] + ms.fit_groups_dtype(NB))
    for m, rec in enumerate(res):
        assert rec.dtype == want, m
        r = np.array(RESIDENT[m], dtype=np.int64)
        for k in ("fit_chi2", "fit_npix"):
            assert np.array_equal(rec[k], _stack(r, k)), (m, k)
        assert np.array_equal(rec["fit_scale_err"], np.sqrt(_stack(r, "fit_var")))       # the weights carry the noise
        assert rec["fit_group"].tolist() == [_group_of(x)[0] for x in r]
    fit_call = [x for x in core.engine.calls if x[0] == "fit_groups"][0][1]
    assert np.array_equal(fit_call["data"], obj.field_images) and np.array_equal(fit_call["weights"], W)
    assert core.engine.calls[0] == ("open", True) and "fit" not in [x[0] for x in core.engine.calls]
    # every shared column has the values of the run without the option
    _, dense, _ = _run(measure=True, fit_flux=True, fit_weights=W, mode="cumulative", max_iterations=3)
    for a, b in zip(res, dense):
        assert a.dtype.names[:len(b.dtype.names)] == b.dtype.names
        for k in b.dtype.names:
            if k != "shifts":
                assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k


def test_the_default_makes_the_calls_it_made():
    """fit_groups=False: the call list of section 7v on a set that does not have the new method at all"""
    assert not hasattr(FittingSet, "fit_flux_groups") and not hasattr(ScriptedSet, "fit_flux_groups")
    for kw in (dict(measure=True, fit_flux=True), dict(measure=True, blendedness=True, fit_flux=True, fit_sky=1, fit_nonneg=True),
               dict(measure=True), dict(measure=False)):
        _, a, ca = _run(engine=FittingEngine, **kw)
        _, b, cb = _run(engine=FittingEngine, fit_groups=False, **kw)
        assert [x[0] for x in ca.engine.calls] == [x[0] for x in cb.engine.calls]
        assert "fit_groups" not in [x[0] for x in cb.engine.calls] and ca.seed_counter == cb.seed_counter
        assert [r.dtype for r in a] == [r.dtype for r in b] and all("fit_group" not in r.dtype.names for r in b)
    calls = [x[0] for x in _run(engine=FittingEngine, measure=True, fit_flux=True, fit_groups=False)[2].engine.calls]
    assert calls.count("fit") == 1 and calls[calls.index("fit"):] == ["fit", "read", "read", "read", "close"]
    import inspect
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch
    params = list(inspect.signature(IterativeDeblendFieldBatch.iterative_catalogue).parameters.values())
    assert params[-1].name == "fit_groups" and params[-1].default is False


def test_refusals():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch
    from debvader_amd.measure import measurement as ms

    W = np.ones((4, F, F, NB))
    both = re.escape(ms.GROUPS_TAKE_NO_SKY_NO_CONSTRAINT)
    assert ms.GROUPS_TAKE_NO_SKY_NO_CONSTRAINT.startswith("fit_groups=True cannot be combined with fit_sky or fit_nonneg")
    for kw, match in ((dict(fit_groups=True), "fit_groups=True needs fit_flux=True"),
                      (dict(measure=True, fit_groups=True), "fit_groups=True needs fit_flux=True"),
                      (dict(fit_flux=True, fit_groups=True), "measure=True"),
                      (dict(measure=True, fit_flux=True, fit_groups=True, fit_sky=0), both),
                      (dict(measure=True, fit_flux=True, fit_groups=True, fit_sky=1, fit_weights=W), both),
                      (dict(measure=True, fit_flux=True, fit_groups=True, fit_nonneg=True), both),
                      (dict(measure=True, fit_flux=True, fit_groups=True, fit_weights=W, sky_sigma=np.ones(NB)),
                       "weights already carry the noise"),
                      (dict(measure=True, fit_flux=True, fit_groups=True, fit_weights=W[:3]), "shape of the data fields"),
                      (dict(measure=True, fit_flux=True, fit_groups=True, min_pivot=0.0), "min_pivot")):
        net = Net(SCRIPT, ROWS)
        net._core.engine = GroupedEngine(SCRIPT, ROWS)
        obj = IterativeDeblendFieldBatch(net, np.zeros((4, F, F, NB)), CS, NB)
        with pytest.raises(ValueError, match=match):
            obj.iterative_catalogue(**kw)
        assert net._core.engine.calls == [], kw                    # refused before the set is opened
    # the text is the one deblend_fields uses for that combination
    src = open(os.path.join(ROOT, "debvader_amd", "deblend", "field_deblender.py")).read()
    assert "raise ValueError(ms.GROUPS_TAKE_NO_SKY_NO_CONSTRAINT)" in src and DeblendFieldBatch is not None


# ---- the definition in the joint order, on the restatement ------------------------------------------------------------------
def _two_pass_field():
    """cs = 31, F = 160, one band, one field.  Pass 0 (resident rows 0 - 3): A at (10, 10) and A2 at (10, 30), which overlap; B
    at (10, 90), 29 columns right of A2's last column: apart; C at (100, 10), alone for good.  Pass 1 (rows 4 - 6): a copy of
    A's model at A's place; a bridge X at (20, 60), which shares column 60 with A2 and column 90 with B: it joins the two
    pass-0 groups; Y at (125, 125), alone.  Joint order = resident order (one field)."""
    cs, Fq = 31, 160
    g = lambda a, b, c, amp: ffo.elliptical_gaussian(cs, (a, b, c), amp=amp).astype(np.float32)[:, :, None]
    A, A2, B, Cg = g(9.0, 1.0, 6.0, 5.0), g(5.0, 0.0, 5.0, 2.0), g(4.0, -1.0, 7.0, 3.0), g(3.0, 0.0, 3.0, 1.0)
    X, Y = g(6.0, 0.5, 4.0, 0.5), g(2.0, 0.0, 2.0, 0.7)
    stamps = np.stack([A, A2, B, Cg, A, X, Y])
    places = np.array([(10, 10), (10, 30), (10, 90), (100, 10), (10, 10), (20, 60), (125, 125)])
    truth = np.array([1.25, 0.75, 1.5, 2.0, 0.0, 1.0, 0.5])           # (the copy carries nothing of its own)
    D = np.zeros((1, Fq, Fq, 1))
    for s, (r, c), t in zip(stamps, places, truth):
        D[0, r:r + cs, c:c + cs] += t * s.astype(np.float64)
    return stamps, places, D, truth


def test_groups_in_the_joint_order_span_passes_and_drop_the_later_copy():
    stamps, places, D, truth = _two_pass_field()
    pass_fptr = [[0, 4], [0, 3]]
    order, fp = _regroup(pass_fptr)
    assert order.tolist() == list(range(7)) and fp.tolist() == [0, 7]
    cs, Fq = stamps.shape[1], D.shape[1]
    # pass 0 alone: {A, A2}, {B}, {C}
    g0, s0 = fgo.groups(places[:4], [0, 4], cs, Fq)
    assert g0.tolist() == [0, 0, 2, 3] and s0.tolist() == [2, 2, 1, 1]
    # both passes: the bridge of pass 1 joins {A, A2} and {B} under the smallest pass-0 row; the copy joins A's group
    group, size = fgo.groups(places[order], fp, cs, Fq)
    assert group.tolist() == [0, 0, 0, 3, 0, 0, 6] and size.tolist() == [5, 5, 5, 1, 5, 5, 1]
    out, per_group = fgo.fit_flux_groups(stamps[order], places[order], fp, D)
    assert out["fit_group"].tolist() == group.tolist() and len(per_group) == 3
    status, scale = out["fit_status"][:, 0], out["fit_scale"][:, 0]
    # inside its group the copy from the LATER pass is dropped; the detection of pass 0 is fitted against D - copy
    assert status.tolist() == [0, 0, 0, 0, 5, 0, 0] and scale[4] == 1.0
    want = truth.copy()
    want[0], want[4] = truth[0] - 1.0, 1.0
    print("grouped joint fit: scale - expected =", scale - want)
    assert np.abs(scale - want).max() <= 1e-10
    # the grouped restatement is the dense one on this field, bit for bit (section 7w)
    dense, _ = ffo.fit_flux(stamps[order], places[order], fp, D)
    for k in ("fit_scale", "fit_var", "fit_gram", "fit_proj", "fit_status"):
        assert np.array_equal(out[k], dense[k], equal_nan=True), k
    # two fields: the rows of the set pass-major, the labels counted from each field's first row in the JOINT order
    pass_fptr = [[0, 2, 4], [0, 1, 3]]                              # field 0: A, A2 | copy; field 1: B, C | X, Y
    res_stamps = stamps[[0, 1, 2, 3, 4, 5, 6]]
    res_places = places[[0, 1, 2, 3, 4, 5, 6]]
    order, fp = _regroup(pass_fptr)
    assert order.tolist() == [0, 1, 4, 2, 3, 5, 6] and fp.tolist() == [0, 3, 7]
    group, size = fgo.groups(res_places[order], fp, cs, Fq)
    assert group.tolist() == [0, 0, 0, 0, 1, 0, 3] and size.tolist() == [3, 3, 3, 2, 1, 2, 1]
    back = np.empty(7, np.int32)
    back[order] = group                                            # resident-row order, as the call returns it
    assert back.tolist() == [0, 0, 0, 1, 0, 0, 3] and res_stamps.shape[0] == 7
