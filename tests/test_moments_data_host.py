"""The adaptive moments on the observed field with the neighbours subtracted without a GPU: the
definition on the numpy restatement of tests/moments_fields_oracle.py, and the host layer (measurement.moments_data_records /
measure_moments_on_fields, DeblendFieldBatch.deblend_fields(moments_data=True), the engine wrappers and the ctypes signatures)
over the stand-ins of tests/stub_moments_data_engine.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests import measure_oracle as mo
from tests import moments_fields_oracle as mf
from tests.stub_measure_engine import stub_catalogue
from tests.stub_moments_data_engine import CS, MKEYS, NB, Net, OracleContext, stub_moments_data
from tests.test_fit_flux_host import _c_types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS21, FH = 21, 48


def _scene():
    """Two fields of 48 pixels, five galaxies on 21-pixel stamps: a pair that overlaps, a stamp over a corner, a stamp wholly
    outside, and one alone in the second field.  T is the composite of the float32 stamps, D is T plus a residual."""
    rng = np.random.default_rng(5)
    P = np.stack([mo.gaussian_stamp(CS21, (4.0 + 0.5 * i, 0.3 * (i % 3 - 1), 5.0 - 0.4 * i), rng.uniform(-1, 1, 2), 1.0 + 0.2 * i)
                  for i in range(5)])[..., None] * np.array([0.5, 0.8, 1.0])
    P = P.astype(np.float32)
    places = np.array([[5, 6], [12, 14], [-8, 38], [-30, 3], [13, 13]])
    fp = [0, 4, 5]
    T = np.zeros((2, FH, FH, 3))
    for m in range(2):
        for i in range(fp[m], fp[m + 1]):
            pr, pc = places[i]
            ra, rz, ca, cz = max(pr, 0), min(pr + CS21, FH), max(pc, 0), min(pc + CS21, FH)
            if rz > ra and cz > ca:
                T[m, ra:rz, ca:cz] += P[i, ra - pr:rz - pr, ca - pc:cz - pc].astype(np.float64)
    D = T + rng.normal(0.0, 0.01, size=T.shape)
    return P, places, fp, T, D


def test_the_child_image_by_hand():
    P, places, fp, T, D = _scene()
    C_, on = mf.child_images(P, places, fp, T, D)
    # inside the field the two roundings in their order; outside it the model; wholly outside: the model's stamp and no pixel
    assert C_[0, 3, 4, 1] == (D[0, 8, 10, 1] - T[0, 8, 10, 1]) + np.float64(P[0, 3, 4, 1]) and on[0].all()
    assert C_[2, 0, 0, 2] == np.float64(P[2, 0, 0, 2]) and not on[2, :8].any() and not on[2, :, 10:].any() and on[2, 8:, :10].all()
    assert np.array_equal(C_[3], P[3].astype(np.float64)) and not on[3].any()
    out = mf.moments_fields(P, places, fp, T, D, band=2)
    assert out["npix_data"].tolist() == [[441] * 3, [441] * 3, [13 * 10] * 3, [0] * 3, [441] * 3] and out["npix_data"].dtype == np.int32
    # D with the bits of T: the child is the stamp, and the rows are measure_oracle's on the stamps
    same = mf.moments_fields(P, places, fp, T, T, band=2)
    want = mo.measure(P, band=2)
    for a, b in (("flux_data", "flux"), ("shape_data", "shape"), ("iters_data", "iters"), ("status_data", "status")):
        assert np.array_equal(same[a], want[b]), a
    assert np.array_equal(out["shape_data"][3], want["shape"][3]) and not np.array_equal(out["shape_data"][0], want["shape"][0])
    # the mask: a NaN, an inf and a huge value of D under weights of 0, a negative value, NaN and inf reach nothing
    W = np.ones_like(D)
    D2 = D.copy()
    for k, (w, d) in enumerate(((0.0, np.nan), (-1.0, np.inf), (np.nan, 1e300), (np.inf, -np.inf))):
        W[0, 10 + k, 12, :] = w
        D2[0, 10 + k, 12, :] = d
    D3 = np.where(mf.counts(W), D, T)
    masked, clean = mf.moments_fields(P, places, fp, T, D2, W), mf.moments_fields(P, places, fp, T, D3)
    for k in ("flux_data", "shape_data", "iters_data", "status_data"):
        assert np.array_equal(masked[k], clean[k]), k
    assert (clean["npix_data"] - masked["npix_data"]).tolist() == [[4] * 3, [0] * 3, [0] * 3, [0] * 3, [0] * 3]
    assert np.array_equal(mf.moments_fields(P, places, fp, T, D, np.ones_like(D))["flux_data"], out["flux_data"])
    # unmasked, a NaN of D under band 2 ends in status 3 on the rows that cover it
    D4 = D.copy()
    D4[0, 15, 17, 2] = np.nan
    assert mf.moments_fields(P, places, fp, T, D4)["status_data"].tolist() == [3, 3, 0, 0, 0]
    hist = []
    mf.moments_fields(P, places, fp, T, D, histories=hist)
    assert len(hist) == 5 and 0.0 < mf.late_contraction(hist[0]) < 1.0


def test_columns_and_records():
    from debvader_amd.measure import measurement as ms

    names = [d[0] for d in ms.moments_data_dtype(3)]
    assert names == ["flux_data", "npix_data", "row_data", "col_data", "Mrr_data", "Mrc_data", "Mcc_data", "iters_data",
                     "status_data", "sigma_data", "e1_data", "e2_data", "flux_data_err"]
    assert ms.moments_data_dtype(6)[0] == ("flux_data", "<f8", (6,)) and ms.moments_data_dtype(6)[1] == ("npix_data", "<i4", (6,))
    s = stub_moments_data(6, 3)
    rec = ms.moments_data_records(*(s[k] for k in MKEYS))
    assert rec.dtype == np.dtype(ms.moments_data_dtype(3)) and np.isnan(rec["flux_data_err"]).all()
    assert np.array_equal(rec["flux_data"], s["flux_data"]) and np.array_equal(rec["npix_data"], s["npix_data"])
    for k, name in enumerate(("row_data", "col_data", "Mrr_data", "Mrc_data", "Mcc_data")):
        assert np.array_equal(rec[name], s["shape_data"][:, k])
    # the derived columns are the catalogue's own, from the same function
    cat = ms.catalogue_records(s["flux_data"], None, s["shape_data"], s["iters_data"], s["status_data"])
    for a, b in (("sigma_data", "sigma"), ("e1_data", "e1"), ("e2_data", "e2")):
        assert np.array_equal(rec[a], cat[b], equal_nan=True), a
    assert np.isnan(rec["sigma_data"][3]) and rec["status_data"][3] == 3 and np.isfinite(rec["e1_data"][[0, 1, 2, 4, 5]]).all()
    assert rec["sigma_data"][0] == np.sqrt(np.sqrt(4.0 * 3.0 - 0.25)) and rec["e1_data"][0] == (3.0 - 4.0) / 7.0
    # sky_sigma: per band, or per field and band
    sig = np.array([0.1, 0.2, 0.3])
    rec = ms.moments_data_records(*(s[k] for k in MKEYS), sky_sigma=sig)
    assert np.array_equal(rec["flux_data_err"], sig * np.sqrt(s["npix_data"].astype(np.float64)))
    rec2 = ms.moments_data_records(*(s[k] for k in MKEYS), sky_sigma=np.stack([sig, 2 * sig]), field_ptr=[0, 4, 6])
    assert np.array_equal(rec2["flux_data_err"][:4], rec["flux_data_err"][:4])
    assert np.array_equal(rec2["flux_data_err"][4:], 2 * rec["flux_data_err"][4:])
    with pytest.raises(ValueError, match="sky_sigma"):
        ms.moments_data_records(*(s[k] for k in MKEYS), sky_sigma=np.ones(2))
    with pytest.raises(ValueError, match="field_ptr"):
        ms.moments_data_records(*(s[k] for k in MKEYS), sky_sigma=sig, field_ptr=[0, 5])
    with pytest.raises(ValueError, match="expected npix_data"):
        ms.moments_data_records(s["flux_data"], s["npix_data"][:, :2], s["shape_data"], s["iters_data"], s["status_data"])
    p = inspect.signature(ms.measure_moments_on_fields).parameters
    assert list(p)[:7] == ["stamps_mean", "places", "data_fields", "model_fields", "weight_fields", "field_ptr", "catalogue"]
    assert p["weight_fields"].default is None and p["band"].default == 2 and p["ctx"].default is None


def test_measure_moments_on_fields_over_the_restatement():
    from debvader_amd.measure import measurement as ms

    P, places, fp, T, D = _scene()
    ctx = OracleContext()
    rec = ms.measure_moments_on_fields(P, places, D, T, field_ptr=fp, ctx=ctx)
    assert rec.dtype == np.dtype(ms.moments_data_dtype(3))
    assert ctx.calls[-1]["moments_fields"] == 5 and ctx.calls[-1]["weights"] is None and ctx.calls[-1]["field_ptr"] == fp
    want = mf.moments_fields(P, places, fp, T, D)
    assert np.array_equal(rec["flux_data"], want["flux_data"]) and np.array_equal(rec["Mrc_data"], want["shape_data"][:, 3])
    assert np.array_equal(rec["npix_data"], want["npix_data"]) and np.isnan(rec["flux_data_err"]).all()
    # one field given without its leading axis; the weights and the parameters are passed on
    W = np.ones_like(D[1])
    W[20:25, 20:25] = 0.0
    one = ms.measure_moments_on_fields(P[4:], places[4:], D[1], T[1], weight_fields=W, sky_sigma=[0.1, 0.1, 0.2], band=1,
                                       sigma0=2.5, max_iter=50, ctx=ctx)
    assert ctx.calls[-1]["weights"] == (FH, FH, 3) and ctx.calls[-1]["band"] == 1 and ctx.calls[-1]["sigma0"] == 2.5
    assert ctx.calls[-1]["max_iter"] == 50 and ctx.calls[-1]["field_ptr"] == [0, 1]
    assert one["npix_data"].tolist() == [[441 - 25] * 3] and np.array_equal(one["flux_data_err"][0], np.array([0.1, 0.1, 0.2]) * np.sqrt(416.0))
    # refused before the context
    n = len(ctx.calls)
    with pytest.raises(ValueError, match="sky_sigma"):
        ms.measure_moments_on_fields(P, places, D, T, field_ptr=fp, sky_sigma=np.ones(2), ctx=ctx)
    with pytest.raises(ValueError, match="the catalogue has 3 rows for 5 stamps"):
        ms.measure_moments_on_fields(P, places, D, T, field_ptr=fp, catalogue=np.recarray((3,), dtype=[("flux", "<f8")]), ctx=ctx)
    assert len(ctx.calls) == n


F = 81
DIST = [np.array([[0.0, 0.0], [5.0, -7.0]]), np.zeros((0, 2)), np.array([[100.0, 0.0], [-3.0, 11.0]]), np.array([[0.0, 40.0]])]


def _batch():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch

    net = Net()
    return net, DeblendFieldBatch(net, np.random.default_rng(3).normal(size=(4, F, F, NB)), CS, NB)


def _engine_calls(net):
    return [c for c in net._core.engine.calls if c[0].startswith("infer")]


def test_deblend_fields_appends_the_moments_data_columns():
    from debvader_amd.deblend import field_deblender as fd
    from debvader_amd.measure import measurement as ms

    B = fd.DeblendFieldBatch
    sig = inspect.signature(B.deblend_fields).parameters
    assert sig["moments_data"].default is False and sig["moments_data"].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig["moments_weights"].default is None and sig["moments_weights"].kind is inspect.Parameter.KEYWORD_ONLY
    assert B.moments_data_columns(NB) == ms.moments_data_dtype(NB)
    keys = [x.key for x in fd._EXTRAS]
    row = fd._EXTRAS[keys.index("moments_data")]
    assert keys.count("moments_data") == 1 and row.refines is None and row.orphans[0][0] == "moments_weights"
    # one row of the table, behind every extra that stands alone: the generic refusals are its own, and it speaks in them
    assert all(x.refines for x in fd._EXTRAS[keys.index("moments_data") + 1:])
    net, b = _batch()
    W = np.random.default_rng(5).uniform(0.5, 2.0, size=(4, F, F, NB))
    base = B.ON_DEVICE_COLUMNS + B.measure_columns(NB)
    s, c = stub_moments_data(3, NB), stub_catalogue(3, NB)
    for rf in (True, False):
        for weights, sky in ((None, None), (W, np.linspace(0.1, 0.6, NB))):
            res = b.deblend_fields(DIST, on_device=True, measure=True, moments_data=True, moments_weights=weights, sky_sigma=sky,
                                   return_fields=rf)
            call = _engine_calls(net)[-1]
            assert call[0] == "infer_fields_measure_moments_data" and call[2] is rf and call[3] is not None and call[5] == 2
            assert call[4] is None if weights is None else np.array_equal(call[4], W)          # the weights are passed on
            want = np.dtype(base + B.moments_data_columns(NB))                                   # exactly these columns
            assert [len(r) for r in res] == [2, 0, 1, 0] and all(r.dtype == want for r in res)
            rec = ms.moments_data_records(*(s[k] for k in MKEYS), sky_sigma=sky, field_ptr=[0, 2, 2, 3, 3])
            cat = ms.catalogue_records(c["flux"], c["flux_err"], c["shape"], c["iters"], c["status"])
            for i, (m, k) in enumerate([(0, 0), (0, 1), (2, 0)]):
                for n in rec.dtype.names:
                    assert np.array_equal(res[m][n][k], rec[n][i], equal_nan=True), n
                for n in cat.dtype.names:                                                        # the catalogue's own stay
                    assert np.array_equal(res[m][n][k], cat[n][i], equal_nan=True), n
            assert np.isnan(res[0]["flux_data_err"]).all() == (sky is None)
    # without it the call and the columns are those of before
    res = b.deblend_fields(DIST, on_device=True, measure=True)
    assert _engine_calls(net)[-1][0] == "infer_fields_measure" and "flux_data" not in res[0].dtype.names


def test_deblend_fields_refuses_moments_data_combinations():
    net, b = _batch()
    W = np.ones((4, F, F, NB))
    on = dict(on_device=True, measure=True)
    md = "moments_data=True"
    for kw, match in ((dict(moments_data=True), md + " needs measure=True and on_device=True"),
                      (dict(moments_data=True, measure=True), md + " needs measure=True and on_device=True.*needs on_device=True"),
                      (dict(moments_data=True, on_device=True), md + " needs measure=True and on_device=True.*needs measure=True"),
                      (dict(moments_weights=W, **on), "moments_weights are the mask.*give moments_data=True too"),
                      (dict(moments_weights=W), "give moments_data=True too"),
                      (dict(moments_data=True, measure_samples=4, **on), md + " cannot be combined with measure_samples"),
                      (dict(moments_data=True, blendedness=True, **on), md + " cannot be combined with blendedness=True"),
                      (dict(moments_data=True, psf=np.ones((21, 21)), **on), md + " cannot be combined with psf"),
                      (dict(moments_data=True, apertures=(3.0,), **on), md + " cannot be combined with apertures"),
                      (dict(moments_data=True, apertures=(3.0,), aperture_data=True, **on), md + " cannot be combined with apertures"),
                      (dict(moments_data=True, fit_flux=True, **on), md + " cannot be combined with fit_flux=True"),
                      (dict(moments_data=True, fit_flux=True, fit_weights=W, **on), md + " cannot be combined with fit_flux=True"),
                      (dict(moments_data=True, fit_flux=True, fit_groups=True, **on), md + " cannot be combined with fit_flux=True"),
                      (dict(moments_data=True, fit_flux=True, fit_sky=0, **on), md + " cannot be combined with fit_flux=True"),
                      (dict(moments_data=True, fit_flux=True, fit_nonneg=True, **on), md + " cannot be combined with fit_flux=True"),
                      (dict(moments_data=True, optimise_positions=True, **on), md + " cannot be combined with optimise_positions=True"),
                      (dict(moments_data=True, epistemic_uncertainty_estimation=True, **on),
                       md + " cannot be combined with epistemic_uncertainty_estimation=True"),
                      (dict(moments_data=True, moments_weights=W[:3], **on), "expected weight fields of the shape of the data fields"),
                      (dict(moments_data=True, sky_sigma=np.ones(NB + 1), **on), "sky_sigma"),
                      (dict(sky_sigma=np.ones(NB), **on), "sky_sigma is the sky noise")):
        with pytest.raises(ValueError, match=match):
            b.deblend_fields(DIST, **kw)
    assert not _engine_calls(net) and net._core.seed_counter == 7          # no engine call, no seed consumed


def test_engine_wrappers_refuse_before_the_library():
    from debvader_amd import engine as E

    P, pl, T = np.zeros((2, 31, 31, 3), np.float32), np.zeros((2, 2), np.int32), np.zeros((1, 40, 40, 3))
    call = lambda *a, **kw: E.Context.scene_moments_fields(object(), *a, **kw)     # noqa: E731
    for bad in (np.zeros((1, 40, 40, 2)), np.zeros((2, 40, 40, 3)), 2.0):
        with pytest.raises(ValueError, match="expected weight fields of the shape of the data fields"):
            call(P, pl, T, T, weight_fields=bad)
    with pytest.raises(ValueError, match="expected data fields"):
        call(P, pl, T, T[:, :39])
    with pytest.raises(ValueError, match="expected data fields"):
        call(P, pl, T[..., :2], T[..., :2])
    with pytest.raises(ValueError, match="expected square stamps"):
        call(P[:, :30], pl, T, T)
    with pytest.raises(ValueError, match="expected places"):
        call(P, pl[:1], T, T)
    with pytest.raises(ValueError, match="field_ptr is needed with 2 fields"):
        call(P, pl, np.zeros((2, 40, 40, 3)), np.zeros((2, 40, 40, 3)))
    with pytest.raises(ValueError, match="field_ptr must"):
        call(P, pl, T, T, field_ptr=[0, 3])
    with pytest.raises(ValueError, match="stamps of 91 pixels: the measurement takes at most 90"):
        call(np.zeros((1, 91, 91, 1), np.float32), pl[:1], np.zeros((1, 40, 40, 1)), np.zeros((1, 40, 40, 1)), band=0)
    for kw, match in ((dict(band=3), "band 3 asked for"), (dict(band=-1), "band"), (dict(sigma0=0.0), "sigma0"),
                      (dict(tol=float("nan")), "tol"), (dict(max_iter=-1), "max_iter"), (dict(max_iter=2.5), "max_iter")):
        with pytest.raises(ValueError, match=match):
            call(P, pl, T, T, **kw)
    # an empty call returns without the library
    empty = call(P[:0], pl[:0], T, T, weight_fields=np.ones((40, 40, 3)))
    assert list(empty) == list(MKEYS) and empty["npix_data"].shape == (0, 3) and empty["npix_data"].dtype == np.int32
    assert empty["shape_data"].shape == (0, 5) and empty["status_data"].dtype == np.int32
    p = inspect.signature(E.Context.scene_moments_fields).parameters
    assert list(p)[1:7] == ["stamps", "places", "model_fields", "data_fields", "weight_fields", "field_ptr"]
    assert list(inspect.signature(E.Engine.scene_moments_fields).parameters)[1:5] == ["stamps", "places", "model_fields", "data_fields"]
    fields = np.zeros((2, 81, 81, 6))
    for kw, match in ((dict(places=None), "places are needed"),
                      (dict(places=None, return_fields=False), "places are needed"),
                      (dict(places=[[0, 0]], weight_fields=fields[:1]), "expected weight fields of the shape of the data fields"),
                      (dict(places=[[0, 0]], sigma0=-1.0), "sigma0"),
                      (dict(places=[[0, 0], [1, 1]]), "placements"),
                      (dict(places=[[0, 0]], band=7), "band")):
        places = kw.pop("places")
        with pytest.raises(ValueError, match=match):
            E.Engine.infer_fields_measure_moments_data(object(), fields, [[0, 0]], [0, 1, 1], places, **kw)


def test_header_binding_and_library_agree_on_the_moments_entry_points():
    from debvader_amd import _lib

    header = open(os.path.join(ROOT, "include", "debvader_hip.h")).read()
    ctype = {"dv_model*": C.c_void_p, "dv_ctx*": C.c_void_p, "double*": C.POINTER(C.c_double), "float*": C.POINTER(C.c_float),
             "int32_t*": C.POINTER(C.c_int32), "int64_t*": C.POINTER(C.c_int64), "int32_t": C.c_int32, "int64_t": C.c_int64,
             "uint64_t": C.c_uint64, "double": C.c_double, "dv_measure_params*": C.POINTER(_lib.DvMeasureParams)}
    for name, nargs in (("dv_scene_moments_fields", 18), ("dv_infer_fields_measure_moments_data", 26)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header, re.S)
        assert m, f"{name} is not declared in include/debvader_hip.h"
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)         # bound: the library exports it
        restype, argtypes = _lib.SIGNATURES[name]
        want = [ctype[t] for t in _c_types(m.group(1))]
        assert restype is C.c_int and len(argtypes) == len(want) == nargs
        for i, (a, w) in enumerate(zip(argtypes, want)):
            assert a is w, (name, i, a, w)
        assert getattr(_lib.lib, name).argtypes == argtypes
    # the 20 arguments of dv_infer_fields_measure, the weights, the five outputs
    pm, p0 = _lib.SIGNATURES["dv_infer_fields_measure_moments_data"][1], _lib.SIGNATURES["dv_infer_fields_measure"][1]
    d, i32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    assert len(p0) == 20 and pm[:20] == p0 and pm[20:] == [d, d, i32, d, i32, i32]
    sm = _lib.SIGNATURES["dv_scene_moments_fields"][1]
    assert sm[13:] == pm[21:] and sm[7:10] == [d, d, d]
    # the existing entry points keep their signatures
    want_len = {"dv_scene_measure": 12, "dv_scene_fit_flux": 16, "dv_scene_fit_flux_weighted": 19, "dv_scene_fit_flux_groups": 21,
                "dv_infer_fields_measure_fit": 26, "dv_infer_fields_measure_fit_weighted": 29,
                "dv_infer_fields_measure_fit_groups": 31, "dv_infer_fields_measure_blend": 22,
                "dv_infer_fields_measure_aper_data": 36, "dv_scene_aperture_fields": 21, "dv_scene_blend": 16}
    for name, n in want_len.items():
        assert len(_lib.SIGNATURES[name][1]) == n, name
    exports = open(os.path.join(ROOT, "debvader_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*dv_\*;", exports) and re.search(r"local:\s*\*;", exports)
    kernel = open(os.path.join(ROOT, "debvader_amd", "csrc", "moments_field.hip")).read()
    for k in ("template <bool MASKED>", "moments_field_kernel", "ms_iterate(", "#pragma clang fp contract(off)"):
        assert k in kernel, k
    assert "getenv" not in kernel and "atomic" not in kernel.replace("No atomics", "")
    assert "moments_field.hip" in open(os.path.join(ROOT, "debvader_amd", "csrc", "Makefile")).read()
    engine = open(os.path.join(ROOT, "debvader_amd", "csrc", "engine.hip")).read()
    assert "launch_moments_field(" in engine and "std::optional<MomentsFieldOut>" in engine
