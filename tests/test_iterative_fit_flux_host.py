"""CPU checks of the joint flux fit of the iterative loop (IterativeDeblendFieldBatch.iterative_catalogue(fit_flux=True),
DESIGN.md section 7v): the order of the unknowns on the numpy restatement of the fit (tests/fit_flux_oracle.py) for a two-pass
scene stated by hand; the host loop against a scripted stand-in for the set, every returned value encoding its resident row
number - the dtype and the order of the columns, the join by resident row across fields that stop after 2, 1, 0 and 3 passes,
the derived columns, the per-field results, the refusals and the calls that are and are not made; and the C ABI of the two new
calls.  No GPU is touched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import fit_flux_oracle as ffo
from tests.test_iterative_batch_host import CS, F, NB, ROOT, ScriptedSet
from tests.test_iterative_catalogue_host import RESIDENT, ROWS, SCRIPT, MeasuringEngine, MeasuringSet, Net

NEW_SYMBOLS = ["dv_field_set_keep_stamps", "dv_field_set_fit_flux"]
CTYPES = {"dv_field_set*": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64, "const double*": C.POINTER(C.c_double),
          "double*": C.POINTER(C.c_double), "int32_t*": C.POINTER(C.c_int32), "int64_t*": C.POINTER(C.c_int64)}


@pytest.fixture(autouse=True)
def _the_joint_fit_exists():
    """Everything here pins section 7v, the restatement included: its order rule is the rule of a call that must exist"""
    from debvader_amd import _lib
    from debvader_amd.engine import FieldSet

    assert all(name in _lib.SIGNATURES for name in NEW_SYMBOLS) and hasattr(FieldSet, "fit_flux")


def test_header_binding_export_map_and_library_have_the_new_symbols():
    from debvader_amd import _lib

    ctypes_of = dict(CTYPES)
    ctypes_of["const dv_fit_flux_params*"] = C.POINTER(_lib.DvFitFluxParams)
    header = open(os.path.join(ROOT, "include", "debvader_hip.h")).read()
    for name in NEW_SYMBOLS:
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl, name
        args = [" ".join(a.split()[:-1]) for a in decl.group(1).replace("\n", " ").split(",")]
        assert args[0] == "dv_field_set*"
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int and argtypes == [ctypes_of[a] for a in args], name
        assert getattr(_lib.lib, name).argtypes == argtypes
    assert len(_lib.SIGNATURES["dv_field_set_fit_flux"][1]) == 24
    exports = open(os.path.join(ROOT, "debvader_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*dv_\*;", exports)
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW_SYMBOLS:
        assert re.search(r"\bT %s$" % name, dyn, re.M), name
    # the library refuses a null handle itself, without a GPU
    assert _lib.lib.dv_field_set_keep_stamps(None, 1) == -1
    assert _lib.lib.dv_field_set_fit_flux(None, 0, None, None, -1, 0, None, 1, *[None] * 16) == -1


# ---- the order of the unknowns, on the restatement ------------------------------------------------------------------------
def _two_pass_scene():
    """cs = 31, F = 64, one band, two fields.  Field 0: the bright galaxy A, found in pass 0 with a model of 0.9 times its
    truth, and the faint galaxy B six pixels away, found in pass 1; the field is D = A + B = model_A / 0.9 + model_B.  Field
    1: a galaxy C alone, found in pass 0 with half its truth.  The set holds the rows pass-major: pass 0 = (A, C), pass 1 =
    (B,), or (B, copy of A's model)."""
    cs, Fq = 31, 64
    A = ffo.elliptical_gaussian(cs, (9.0, 1.0, 6.0), amp=5.0).astype(np.float32)[:, :, None]
    B = ffo.elliptical_gaussian(cs, (3.0, 0.0, 3.0), amp=0.25).astype(np.float32)[:, :, None]
    Cg = ffo.elliptical_gaussian(cs, (4.0, -1.0, 5.0), amp=2.0).astype(np.float32)[:, :, None]
    pA, pB, pC = (14, 12), (14, 18), (-3, 40)                     # (C hangs over the top edge)
    D = np.zeros((2, Fq, Fq, 1))
    D[0, pA[0]:pA[0] + cs, pA[1]:pA[1] + cs] += A.astype(np.float64) / 0.9
    D[0, pB[0]:pB[0] + cs, pB[1]:pB[1] + cs] += B.astype(np.float64)
    D[1, 0:cs - 3, pC[1]:Fq] += 2.0 * Cg.astype(np.float64)[3:, :Fq - pC[1]]
    return (A, B, Cg), (pA, pB, pC), D


def _regroup(pass_fptr):
    """order[dst] = resident row: field by field, pass after pass inside a field, the in-pass order last; the joint field_ptr"""
    M = len(pass_fptr[0]) - 1
    base = np.concatenate([[0], np.cumsum([fp[-1] for fp in pass_fptr])])
    order = [base[p] + i for m in range(M) for p, fp in enumerate(pass_fptr) for i in range(fp[m], fp[m + 1])]
    counts = np.sum([np.diff(fp) for fp in pass_fptr], axis=0)
    return np.array(order, dtype=np.int64), np.concatenate([[0], np.cumsum(counts)])


def test_rows_in_pass_order_recover_both_galaxies_and_drop_the_later_copy():
    (A, B, Cg), (pA, pB, pC), D = _two_pass_scene()
    # resident rows, pass-major: A, C | B
    stamps, places = np.stack([A, Cg, B]), np.array([pA, pC, pB])
    order, fp = _regroup([[0, 1, 2], [0, 1, 1]])
    assert order.tolist() == [0, 2, 1] and fp.tolist() == [0, 2, 3]
    out, _ = ffo.fit_flux(stamps[order], places[order], fp, D)
    scale = np.empty(3)
    scale[order] = out["fit_scale"][:, 0]                          # back to resident-row order
    assert out["fit_status"].ravel().tolist() == [0, 0, 0]
    print("joint fit of (A, B), C alone: scale - expected =", scale - np.array([1 / 0.9, 2.0, 1.0]))
    assert abs(scale[0] - 1 / 0.9) <= 1e-11 and abs(scale[2] - 1.0) <= 1e-11 and abs(scale[1] - 2.0) <= 1e-11
    # B fitted alone against D takes A's light under its footprint
    alone, _ = ffo.fit_flux(stamps[2:3], places[2:3], [0, 1], D[:1])
    assert abs(alone["fit_scale"][0, 0] - 1.0) > 0.02
    # an exact copy of A's model as a second row of pass 1: A, C | B, copy
    stamps, places = np.stack([A, Cg, B, A]), np.array([pA, pC, pB, pA])
    order, fp = _regroup([[0, 1, 2], [0, 2, 2]])
    assert order.tolist() == [0, 2, 3, 1] and fp.tolist() == [0, 3, 4]
    out, _ = ffo.fit_flux(stamps[order], places[order], fp, D)
    scale, status = np.empty(4), np.empty(4, np.int32)
    scale[order], status[order] = out["fit_scale"][:, 0], out["fit_status"][:, 0]
    assert status.tolist() == [0, 0, 0, 5] and scale[3] == 1.0     # the copy from the later pass is the one dropped
    # ... and the earlier detection is fitted against D - copy = (1 / 0.9 - 1) model_A + model_B
    assert abs(scale[0] - (1 / 0.9 - 1.0)) <= 1e-11 and abs(scale[2] - 1.0) <= 1e-11
    # the other order would drop the detection of pass 0
    swapped, _ = ffo.fit_flux(stamps[[3, 2, 0]], places[[3, 2, 0]], [0, 3], D[:1])
    assert swapped["fit_status"][:, 0].tolist() == [0, 0, 5]


# ---- the host loop against a scripted set ---------------------------------------------------------------------------------
def _fit_row(r):
    """What the scripted fit returns for resident row r, (bands,) each"""
    b = np.arange(NB)
    return dict(fit_scale=2.0 + r + b / 16.0, fit_var=(r + 1.0) / 64.0 + b, fit_gram=r + 3.0 + b, fit_proj=2.0 * r + 1.0 - b,
                fit_status=np.where((r + b) % 7 == 6, 5, 0).astype(np.int32), fit_chi2=r + 0.125 + b,
                fit_npix=(r + 100 * b).astype(np.int32), fit_scale_free=-(r + 1.0) - b, fit_clamped=((r + b) % 2).astype(np.int32),
                fit_dual=0.5 * r + b)


class FittingSet(MeasuringSet):
    """MeasuringSet plus the two calls of section 7v; the per-field arrays encode the field: sky_coef[m, b, t] = m + b / 8 + t /
    64, sky_cov[m, b] = (m + 1) I, sky_npix = 1000 + m, nonneg_iters = m + 1."""

    def keep_stamps(self, on=True):
        assert not self.closed
        self.owner.calls.append(("keep", bool(on)))

    def fit_flux(self, data_fields=None, weight_fields=None, sky_order=None, nonneg=False, min_pivot=1e-8, max_iter=100,
                 scratch_bytes=256 << 20):
        assert not self.closed
        self.owner.calls.append(("fit", dict(data=data_fields, weights=weight_fields, sky_order=sky_order, nonneg=nonneg,
                                             min_pivot=min_pivot)))
        rows = [_fit_row(r) for r in range(self.rows)]
        keys = ["fit_scale", "fit_var", "fit_gram", "fit_proj", "fit_status"]
        keys += ["fit_chi2", "fit_npix"] if weight_fields is not None else []
        keys += ["fit_scale_free", "fit_clamped", "fit_dual"] if nonneg else []
        out = {k: np.array([row[k] for row in rows]).reshape(self.rows, NB) for k in keys}
        M = self.M
        if sky_order is not None:
            q = 1 if sky_order == 0 else 3
            m, b, t = np.arange(M)[:, None, None], np.arange(NB)[None, :, None], np.arange(q)[None, None, :]
            out.update(sky_coef=m + b / 8.0 + t / 64.0, sky_cov=(np.arange(M) + 1.0)[:, None, None, None] * np.eye(q) * np.ones((M, NB, 1, 1)),
                       sky_status=np.zeros((M, NB, q), np.int32), sky_npix=np.repeat(1000 + np.arange(M), NB).reshape(M, NB))
        if nonneg:
            out.update(nonneg_iters=np.repeat(1 + np.arange(M), NB).reshape(M, NB).astype(np.int32),
                       nonneg_status=np.zeros((M, NB), np.int32))
        return out


class FittingEngine(MeasuringEngine):
    def open_field_set(self, fields, cumulative=False):
        self.calls.append(("open", bool(cumulative)))
        self.sets.append(FittingSet(self, np.asarray(fields), cumulative))
        return self.sets[-1]


def _run(script=SCRIPT, rows=ROWS, **kw):
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch

    net = Net(script, rows)
    net._core.engine = FittingEngine(script, rows)
    fields = np.random.default_rng(1).normal(size=(len(script), F, F, NB))
    obj = IterativeDeblendFieldBatch(net, fields, CS, NB)
    return obj, obj.iterative_catalogue(**kw), net._core


def _flux(r):
    return np.outer(r + 1.0, np.arange(1, NB + 1))                 # (what MeasuringSet measures for resident row r)


def _stack(rows, key):
    return np.array([_fit_row(r)[key] for r in rows]).reshape(len(rows), NB)


def test_columns_join_and_derived_values():
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch as B
    from debvader_amd.measure import measurement as ms

    sky = np.linspace(0.5, 1.0, NB)
    obj, res, core = _run(measure=True, blendedness=True, fit_flux=True, sky_sigma=sky, min_pivot=1e-6)
    assert [len(m) for m in obj.mse] == [2, 1, 0, 3]
    names = [n for n, *_ in ms.fit_flux_dtype(NB)]
    assert names == ["fit_scale", "fit_var", "fit_gram", "fit_proj", "fit_status", "flux_fit", "fit_scale_alone",
                     "fit_independence", "fit_scale_err", "flux_fit_err"]
    want = np.dtype(B.COLUMNS + B.catalogue_columns(NB, True) + ms.fit_flux_dtype(NB))
    for m, rec in enumerate(res):
        assert rec.dtype == want and isinstance(rec, np.recarray), m
        r = np.array(RESIDENT[m], dtype=np.int64)
        assert len(rec) == len(r)
        for k in ("fit_scale", "fit_var", "fit_gram", "fit_proj", "fit_status"):
            assert np.array_equal(rec[k], _stack(r, k)), (m, k)
        assert np.array_equal(rec["flux"], _flux(r))
        assert np.array_equal(rec["flux_fit"], _stack(r, "fit_scale") * _flux(r))     # the flux of the row's own pass
        assert np.array_equal(rec["fit_scale_alone"], _stack(r, "fit_proj") / _stack(r, "fit_gram"))
        assert np.array_equal(rec["fit_scale_err"], sky[None, :] * np.sqrt(_stack(r, "fit_var")))
        assert np.array_equal(rec["flux_fit_err"], sky[None, :] * np.sqrt(_stack(r, "fit_var")) * np.abs(_flux(r)))
        assert np.array_equal(rec["blend_model"], r + 0.25)                             # the other end-of-loop join still holds
    assert obj.sky_fit is None and obj.nonneg_fit is None
    # sky_sigma per field and band
    sky2 = np.arange(1, 4 * NB + 1, dtype=np.float64).reshape(4, NB)
    _, res2, _ = _run(measure=True, fit_flux=True, sky_sigma=sky2)
    for m, rec in enumerate(res2):
        r = np.array(RESIDENT[m], dtype=np.int64)
        assert rec.dtype == np.dtype(B.COLUMNS + B.catalogue_columns(NB, False) + ms.fit_flux_dtype(NB))
        assert np.array_equal(rec["fit_scale_err"], sky2[m][None, :] * np.sqrt(_stack(r, "fit_var"))), m
    # without it the errors are NaN
    _, res3, _ = _run(measure=True, fit_flux=True)
    assert all(np.isnan(rec["fit_scale_err"]).all() and np.isnan(rec["flux_fit_err"]).all() for rec in res3)
    # the calls: the switch once, before the first pass; every pass with the child sums although blendedness is off; one fit,
    # before the reads and the close
    for c, blended in ((core, True), (_run(measure=True, fit_flux=True)[2], False)):
        calls = [x[0] for x in c.engine.calls]
        assert calls.count("keep") == 1 and calls.index("keep") == calls.index("open") + 1 < calls.index("detect")
        assert all(x[1]["blend"] is True for x in c.engine.calls if x[0] == "measure") and calls.count("measure") == 3
        assert calls.count("fit") == 1 and calls.count("sums") == int(blended)
        tail = calls[calls.index("fit"):]
        assert tail == ["fit", "read", "read", "read", "close"]
        if blended:
            assert calls.index("sums") == calls.index("fit") - 1
    fit_call = [x for x in core.engine.calls if x[0] == "fit"][0][1]
    assert fit_call == dict(data=None, weights=None, sky_order=None, nonneg=False, min_pivot=1e-6)


def test_weights_sky_and_nonneg_columns_and_the_per_field_results():
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch as B
    from debvader_amd.measure import measurement as ms

    W = np.random.default_rng(2).uniform(0.5, 2.0, size=(4, F, F, NB))
    obj, res, core = _run(measure=True, blendedness=True, fit_flux=True, fit_weights=W, fit_sky=1, fit_nonneg=True,
                          mode="cumulative", max_iterations=3)
    want = np.dtype(B.COLUMNS + B.catalogue_columns(NB, True) + ms.fit_flux_dtype(NB)
                    + [("fit_chi2", "<f8", (NB,)), ("fit_npix", "<i4", (NB,))] + ms.fit_sky_dtype(NB) + ms.fit_nonneg_dtype(NB))
    assert [n for n, *_ in ms.fit_sky_dtype(NB)] == ["fit_sky", "fit_sky_err"]
    assert [n for n, *_ in ms.fit_nonneg_dtype(NB)] == ["fit_scale_free", "flux_fit_free", "fit_clamped", "fit_dual"]
    po = int((F - CS) / 2)
    for m, rec in enumerate(res):
        assert rec.dtype == want, m
        r = np.array(RESIDENT[m], dtype=np.int64)
        assert len(rec) == len(r)
        for k in ("fit_chi2", "fit_npix", "fit_scale_free", "fit_clamped", "fit_dual"):
            assert np.array_equal(rec[k], _stack(r, k)), (m, k)
        assert np.array_equal(rec["flux_fit_free"], _stack(r, "fit_scale_free") * _flux(r))
        assert np.array_equal(rec["fit_scale_err"], np.sqrt(_stack(r, "fit_var")))       # the weights carry the noise
        # the plane of field m at the centre pixel of every stamp, in the basis of section 7t
        pr = po + rec["galaxy_distances_to_center_x"].astype(np.int64) + CS // 2
        pc = po + rec["galaxy_distances_to_center_y"].astype(np.int64) + CS // 2
        basis = np.stack([np.ones(len(r)), (2 * pr - F + 1) / float(F), (2 * pc - F + 1) / float(F)], axis=1)
        coef = m + np.arange(NB)[:, None] / 8.0 + np.arange(3)[None, :] / 64.0          # (bands, 3)
        assert np.allclose(rec["fit_sky"], basis @ coef.T, rtol=1e-14, atol=0)
        assert np.allclose(rec["fit_sky_err"], np.sqrt((m + 1.0) * (basis ** 2).sum(axis=1))[:, None] * np.ones(NB), rtol=1e-14)
    assert sorted(obj.sky_fit) == ["sky_coef", "sky_cov", "sky_npix", "sky_status"] and obj.sky_fit["sky_coef"].shape == (4, NB, 3)
    assert obj.sky_fit["sky_npix"][:, 0].tolist() == [1000, 1001, 1002, 1003]
    assert sorted(obj.nonneg_fit) == ["nonneg_iters", "nonneg_status"] and obj.nonneg_fit["nonneg_iters"][:, 0].tolist() == [1, 2, 3, 4]
    # a cumulative set keeps no base: the call receives the fields; the weights and the order go through
    fit_call = [x for x in core.engine.calls if x[0] == "fit"][0][1]
    assert np.array_equal(fit_call["data"], obj.field_images) and np.array_equal(fit_call["weights"], W)
    assert fit_call["sky_order"] == 1 and fit_call["nonneg"] is True and core.engine.calls[0] == ("open", True)
    # a later run without the per-field extras forgets them
    obj.iterative_catalogue(measure=True, fit_flux=True)
    assert obj.sky_fit is None and obj.nonneg_fit is None


def test_return_fields_false_reads_nothing():
    obj, res, core = _run(measure=True, fit_flux=True, fit_sky=0, return_fields=False)
    calls = [x[0] for x in core.engine.calls]
    assert "read" not in calls and calls[-2:] == ["fit", "close"] and "sums" not in calls
    full = _run(measure=True, fit_flux=True, fit_sky=0)[1]
    for a, b in zip(res, full):
        for k in a.dtype.names:
            if k != "shifts":
                assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k


def test_defaults_make_the_calls_they_always_made():
    from tests.test_iterative_catalogue_host import _run as run_before

    for kw in (dict(), dict(measure=True), dict(measure=True, blendedness=True, return_fields=False)):
        _, res, core = _run(**kw) if kw else _run(measure=False)
        _, res0, core0 = run_before(SCRIPT, ROWS, **kw)
        a, b = core.engine.calls, core0.engine.calls
        assert [x[0] for x in a] == [x[0] for x in b] and "keep" not in [x[0] for x in a] and "fit" not in [x[0] for x in a]
        assert [x[1] for x in a if x[0] == "measure"] == [x[1] for x in b if x[0] == "measure"]
        assert core.seed_counter == core0.seed_counter
        assert [r.dtype for r in res] == [r.dtype for r in res0]
    # the plain loop runs on a set that has neither call
    assert not hasattr(ScriptedSet, "keep_stamps") and not hasattr(ScriptedSet, "fit_flux")


def test_refusals():
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch

    W = np.ones((4, F, F, NB))
    for kw, match in ((dict(fit_flux=True), "measure=True"),
                      (dict(measure=True, fit_weights=W), "fit_weights needs fit_flux=True"),
                      (dict(measure=True, fit_sky=0), "fit_sky needs fit_flux=True"),
                      (dict(measure=True, fit_nonneg=True), "fit_nonneg=True needs fit_flux=True"),
                      (dict(measure=True, sky_sigma=np.ones(NB)), "sky_sigma needs fit_flux=True"),
                      (dict(measure=True, fit_flux=True, fit_weights=W, sky_sigma=np.ones(NB)), "weights already carry the noise"),
                      (dict(measure=True, fit_flux=True, fit_weights=W[:3]), "shape of the data fields"),
                      (dict(measure=True, fit_flux=True, fit_sky=2), "sky_order"),
                      (dict(measure=True, fit_flux=True, fit_sky=True), "sky_order"),
                      (dict(measure=True, fit_flux=True, sky_sigma=np.ones(NB + 1)), "sky_sigma must have shape"),
                      (dict(measure=True, fit_flux=True, sky_sigma=-np.ones(NB)), "finite and positive"),
                      (dict(measure=True, fit_flux=True, min_pivot=1.0), "min_pivot")):
        net = Net(SCRIPT, ROWS)
        net._core.engine = FittingEngine(SCRIPT, ROWS)
        obj = IterativeDeblendFieldBatch(net, np.zeros((4, F, F, NB)), CS, NB)
        with pytest.raises(ValueError, match=match):
            obj.iterative_catalogue(**kw)
        assert net._core.engine.calls == [], kw                    # refused before the set is opened
