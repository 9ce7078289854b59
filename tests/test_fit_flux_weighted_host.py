"""The weighted flux fit without a GPU: the definition on the numpy restatement of
tests/fit_flux_weighted_oracle.py - unit and constant weights, masks with NaN under them, a mask against a crop, a wholly masked
galaxy, the error and chi-square formulas against heteroscedastic noise realisations - and the host layer
(measurement.fit_flux_records / fit_fluxes_weighted, DeblendFieldBatch.deblend_fields(fit_weights=...), the engine wrappers and
the ctypes signatures) over the stand-ins of tests/stub_fit_flux_weighted_engine.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests import fit_flux_oracle as fo
from tests import fit_flux_weighted_oracle as fw
from tests.stub_fit_flux_weighted_engine import CS, KEYS, NB, WKEYS, Net, OracleContext, stub_fit_flux_weighted
from tests.stub_measure_engine import stub_catalogue
from tests.test_fit_flux_host import CS31, F64, M1, O1, _c_types, _pair, _paste, _stamp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_unit_weights_are_the_unweighted_fit_bit_for_bit():
    P, places, D, _ = _pair()
    D = D + np.random.default_rng(1).normal(0.0, 0.05, size=D.shape)
    want, wf = fo.fit_flux(P, places, [0, 2], D[None])
    got, gf = fw.fit_flux(P, places, [0, 2], D[None], np.ones_like(D)[None])
    for k in KEYS + ("gram_abs", "proj_abs"):
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    assert np.array_equal(gf[0]["G"], wf[0]["G"]) and np.array_equal(gf[0]["h"], wf[0]["h"])
    # every pixel counts: the clipped stamp
    assert (got["fit_npix"] == CS31 * CS31).all() and got["fit_npix"].dtype == np.int32
    assert np.isfinite(got["fit_chi2"]).all() and (got["fit_chi2"] > 0).all()


def test_a_constant_weight_scales_the_variance_and_nothing_else():
    P, places, D, _ = _pair()
    D = D + np.random.default_rng(2).normal(0.0, 0.05, size=D.shape)
    one, _ = fw.fit_flux(P, places, [0, 2], D[None], np.ones_like(D)[None])
    for c in (3.7, 0.25):
        got, _ = fw.fit_flux(P, places, [0, 2], D[None], np.full_like(D, c)[None])
        assert np.array_equal(got["fit_status"], one["fit_status"])
        assert np.abs(got["fit_scale"] - one["fit_scale"]).max() <= 1e-12 * np.abs(one["fit_scale"]).max()
        assert np.abs(got["fit_var"] * c - one["fit_var"]).max() <= 1e-12 * one["fit_var"].max()
        assert np.abs(got["fit_chi2"] / c - one["fit_chi2"]).max() <= 1e-12 * one["fit_chi2"].max()
        assert np.array_equal(got["fit_npix"], one["fit_npix"])
    quarter, _ = fw.fit_flux(P, places, [0, 2], D[None], np.full_like(D, 0.25)[None])
    # a power of two scales every term exactly
    assert np.array_equal(quarter["fit_gram"], 0.25 * one["fit_gram"]) and np.array_equal(quarter["fit_proj"], 0.25 * one["fit_proj"])


def test_masked_pixels_and_the_nan_under_them_reach_no_sum():
    P, places, D, truth = _pair(sep=6, bias=0.9)
    rng = np.random.default_rng(3)
    W = rng.uniform(0.25, 4.0, size=D.shape)
    masked = rng.random(D.shape) < 0.3
    W[masked] = 0.0
    D = D.copy()
    D[masked] = np.nan
    got, _ = fw.fit_flux(P, places, [0, 2], D[None], W[None])
    assert (got["fit_status"] == 0).all()
    assert np.abs(got["fit_scale"] - truth[:, None]).max() < 1e-11
    assert np.isfinite(got["fit_gram"]).all() and np.isfinite(got["fit_proj"]).all()
    for i, (pr, pc) in enumerate(places):
        sl = (slice(pr, pr + CS31), slice(pc, pc + CS31))
        on = ~masked[sl]
        assert np.array_equal(got["fit_npix"][i], on.sum(axis=(0, 1)))
        yard = np.where(on, W[sl] * np.where(on, D[sl], 0.0) ** 2, 0.0).sum(axis=(0, 1))
        assert (got["fit_chi2"][i] <= 1e-20 * yard).all(), (got["fit_chi2"][i], yard)
    # negative, infinite and NaN weights mask like zero
    W2 = W.copy()
    W2[masked] = rng.choice([-1.0, np.inf, np.nan, -np.inf, 0.0], size=int(masked.sum()))
    again, _ = fw.fit_flux(P, places, [0, 2], D[None], W2[None])
    for k in WKEYS:
        assert np.array_equal(again[k], got[k]), k


def test_a_mask_is_a_crop():
    P = _stamp(M1, O1)[None]
    places = np.array([[20, 11]])
    D = _paste(F64, P, places, [1.3]) + np.random.default_rng(5).normal(0.0, 0.05, size=(F64, F64, 3))
    Fc = 40                                                        # the stamp covers rows 20 .. 50: rows 40 .. are masked
    W = np.zeros_like(D)
    W[:Fc, :Fc] = 1.0
    got, _ = fw.fit_flux(P, places, [0, 1], D[None], W[None])
    want, _ = fo.fit_flux(P, places, [0, 1], D[None, :Fc, :Fc])
    assert np.array_equal(got["fit_status"], want["fit_status"]) and (got["fit_status"] == 0).all()
    assert np.abs(got["fit_scale"] - want["fit_scale"]).max() <= 1e-12 * np.abs(want["fit_scale"]).max()
    assert np.abs(got["fit_var"] - want["fit_var"]).max() <= 1e-12 * want["fit_var"].max()
    assert (got["fit_npix"] == (Fc - 20) * (Fc - 11)).all()


def test_a_wholly_masked_galaxy_is_ineligible():
    P, places, D, truth = _pair(sep=13)
    W = np.ones_like(D)
    pr, pc = places[1]
    W[pr:pr + CS31, pc:pc + CS31, :] = 0.0                          # all of galaxy 1 and part of galaxy 0
    W[:, :, 2] = np.nan                                             # ... and band 2 everywhere
    got, _ = fw.fit_flux(P, places, [0, 2], D[None], W[None])
    assert got["fit_status"].tolist() == [[0, 0, 4], [4, 4, 4]]
    assert (got["fit_npix"][1] == 0).all() and np.isnan(got["fit_chi2"][1]).all() and np.isnan(got["fit_scale"][1]).all()
    assert (got["fit_gram"][1] == 0.0).all() and (got["fit_proj"][1] == 0.0).all()
    assert got["fit_npix"][0].tolist() == [CS31 * 13, CS31 * 13, 0] and np.isnan(got["fit_chi2"][0, 2])
    # galaxy 0 is fitted on the columns galaxy 1 does not reach: only its own light lies there
    assert np.isfinite(got["fit_chi2"][0, :2]).all() and np.abs(got["fit_scale"][0, :2] - truth[0]).max() < 0.05


def test_heteroscedastic_noise_the_variance_and_the_chi_square():
    """One symmetric Gaussian over the middle of a field whose left half has sigma 0.05 and whose right half 0.2, 400 noise
    realisations: sqrt(fit_var) is the scatter of the weighted amplitude (15 %: the margin of section 7q; the standard error of
    a standard deviation at 400 samples is 3.5 %), the weighted fit scatters less than 0.7 of the unweighted one (analytically
    sqrt(0.0047 / 0.02125) = 0.47) and the mean chi-square lies within 4 sqrt(2 dof / 400) of dof = fit_npix - 1."""
    cs, F, R = 30, 40, 400
    P = fo.elliptical_gaussian(cs, (6.0, 0.0, 6.0))[None, :, :, None].astype(np.float32)
    places = np.array([[4, F // 2 - cs // 2]])                      # columns 5 .. 34: the centre between columns 19 and 20
    sigma = np.full((F, F, 1), 0.05)
    sigma[:, F // 2:] = 0.2
    W = 1.0 / sigma ** 2
    model = _paste(F, P, places)
    rng = np.random.default_rng(17)
    aw, au, chi = np.zeros(R), np.zeros(R), np.zeros(R)
    for k in range(R):
        D = model + rng.normal(size=model.shape) * sigma
        w, _ = fw.fit_flux(P, places, [0, 1], D[None], W[None])
        u, _ = fo.fit_flux(P, places, [0, 1], D[None])
        aw[k], au[k], chi[k] = w["fit_scale"][0, 0], u["fit_scale"][0, 0], w["fit_chi2"][0, 0]
    dof = int(w["fit_npix"][0, 0]) - 1
    assert dof == cs * cs - 1
    sw, su, pred = aw.std(ddof=1), au.std(ddof=1), float(np.sqrt(w["fit_var"][0, 0]))
    print(f"weighted scatter {sw:.5f} against sqrt(fit_var) {pred:.5f}; unweighted {su:.5f}, ratio {sw / su:.3f}; "
          f"mean chi2 {chi.mean():.1f} for {dof} degrees of freedom")
    assert abs(sw / pred - 1.0) < 0.15
    assert sw < 0.7 * su
    assert abs(chi.mean() - dof) < 4.0 * np.sqrt(2.0 * dof / R)
    assert abs(aw.mean() - 1.0) < 4.0 * pred / np.sqrt(R)


# ---- the host layer over the stand-ins ----------------------------------------------------------------------------------------
def test_columns_and_the_error_columns_with_weights():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch
    from debvader_amd.measure import measurement as ms

    nb = 4
    cols = ms.fit_flux_weighted_dtype(nb)
    assert cols == ms.fit_flux_dtype(nb) + [("fit_chi2", "<f8", (nb,)), ("fit_npix", "<i4", (nb,))]
    assert DeblendFieldBatch.fit_flux_weighted_columns(nb) == cols
    sig = inspect.signature(ms.fit_flux_records).parameters
    assert list(sig)[-3:] == ["fit_chi2", "fit_npix", "weighted"] and sig["weighted"].default is False
    assert sig["fit_chi2"].default is None and sig["fit_npix"].default is None
    n = 7
    f = stub_fit_flux_weighted(n, nb)
    flux = stub_catalogue(n, nb)["flux"] - 2.0
    rec = ms.fit_flux_records(*(f[k] for k in KEYS), flux, fit_chi2=f["fit_chi2"], fit_npix=f["fit_npix"])
    assert rec.dtype == np.dtype(cols)
    assert np.array_equal(rec["fit_scale_err"], np.sqrt(f["fit_var"]), equal_nan=True)
    assert np.array_equal(rec["flux_fit_err"], np.sqrt(f["fit_var"]) * np.abs(flux), equal_nan=True)
    assert np.array_equal(rec["fit_chi2"], f["fit_chi2"], equal_nan=True) and np.array_equal(rec["fit_npix"], f["fit_npix"])
    assert rec["fit_npix"].dtype == np.int32 and np.isnan(rec["fit_scale_err"][1, 0]) and np.isnan(rec["fit_chi2"][4, -1])
    # weighted=True alone: the columns of the unweighted records, the errors from the weights
    five = ms.fit_flux_records(*(f[k] for k in KEYS), flux, weighted=True)
    assert five.dtype == np.dtype(ms.fit_flux_dtype(nb))
    for k in five.dtype.names:
        assert np.array_equal(five[k], rec[k], equal_nan=True), k
    plain = ms.fit_flux_records(*(f[k] for k in KEYS), flux)
    assert np.isnan(plain["fit_scale_err"]).all() and np.array_equal(plain["flux_fit"], rec["flux_fit"], equal_nan=True)
    for kw in (dict(weighted=True), dict(fit_chi2=f["fit_chi2"], fit_npix=f["fit_npix"])):
        with pytest.raises(ValueError, match="weights already carry the noise"):
            ms.fit_flux_records(*(f[k] for k in KEYS), flux, sky_sigma=np.ones(nb), **kw)
    with pytest.raises(ValueError, match="go together"):
        ms.fit_flux_records(*(f[k] for k in KEYS), flux, fit_chi2=f["fit_chi2"])


def test_fit_fluxes_weighted_over_the_restatement():
    from debvader_amd.measure import measurement as ms

    sig = inspect.signature(ms.fit_fluxes_weighted).parameters
    assert list(sig)[:4] == ["stamps_mean", "places", "data_fields", "weight_fields"]
    P, places, D, truth = _pair()
    rng = np.random.default_rng(8)
    W = rng.uniform(0.25, 4.0, size=D.shape)
    W[rng.random(D.shape) < 0.2] = 0.0
    ctx = OracleContext()
    rec = ms.fit_fluxes_weighted(P, places, D, W, ctx=ctx)           # one field and its weights given as (F, F, bands)
    assert ctx.calls[-1] == dict(fit_flux_weighted=2, fields=1, min_pivot=1e-8, weights=(1, F64, F64, 3), field_ptr=[0, 2])
    assert rec.dtype == np.dtype(ms.fit_flux_weighted_dtype(3))
    flux = P.sum(axis=(1, 2), dtype=np.float64)
    assert np.abs(rec["fit_scale"] - truth[:, None]).max() < 1e-11 and np.array_equal(rec["flux_fit"], rec["fit_scale"] * flux)
    assert np.array_equal(rec["fit_scale_err"], np.sqrt(rec["fit_var"])) and (rec["fit_scale_err"] > 0).all()
    assert np.array_equal(rec["flux_fit_err"], rec["fit_scale_err"] * np.abs(flux))
    want, _ = fw.fit_flux(P, places, [0, 2], D[None], W[None])
    assert np.array_equal(rec["fit_chi2"], want["fit_chi2"]) and np.array_equal(rec["fit_npix"], want["fit_npix"])
    # two fields and the catalogue's flux
    cat = np.recarray((4,), dtype=[("flux", "<f8", (3,))])
    cat["flux"] = np.arange(12.0).reshape(4, 3) - 3.0
    P4, pl4 = np.concatenate([P, P[::-1]]), np.concatenate([places, places[::-1]])
    rec = ms.fit_fluxes_weighted(P4, pl4, np.stack([D, D]), np.stack([W, W]), field_ptr=[0, 2, 4], catalogue=cat, min_pivot=1e-6,
                                 ctx=ctx)
    assert ctx.calls[-1] == dict(fit_flux_weighted=4, fields=2, min_pivot=1e-6, weights=(2, F64, F64, 3), field_ptr=[0, 2, 4])
    assert np.array_equal(rec["flux_fit"], rec["fit_scale"] * cat["flux"])
    assert np.array_equal(rec["flux_fit_err"], np.sqrt(rec["fit_var"]) * np.abs(cat["flux"]))
    # the unweighted call is what it was
    plain = ms.fit_fluxes(P, places, D, ctx=ctx)
    assert ctx.calls[-1] == dict(fit_flux=2, fields=1, min_pivot=1e-8, field_ptr=[0, 2]) and "fit_chi2" not in plain.dtype.names
    n_calls = len(ctx.calls)
    with pytest.raises(ValueError, match="weights already carry the noise"):
        ms.fit_fluxes_weighted(P, places, D, W, sky_sigma=[0.1, 0.1, 0.1], ctx=ctx)
    for bad in (W[:, :, :2], W[:-1], np.stack([W, W]), W[0], 1.0):
        with pytest.raises(ValueError, match="expected weight fields of the shape of the data fields"):
            ms.fit_fluxes_weighted(P, places, D, bad, ctx=ctx)
    with pytest.raises(ValueError, match="weight_fields must be given"):
        ms.fit_fluxes_weighted(P, places, D, None, ctx=ctx)
    assert len(ctx.calls) == n_calls


F = 81
DIST = [np.array([[0.0, 0.0], [5.0, -7.0]]), np.zeros((0, 2)), np.array([[100.0, 0.0], [-3.0, 11.0]]), np.array([[0.0, 40.0]])]


def _batch():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch

    net = Net()
    return net, DeblendFieldBatch(net, np.random.default_rng(3).normal(size=(4, F, F, NB)), CS, NB)


def _engine_calls(net):
    return [c for c in net._core.engine.calls if c[0].startswith("infer")]


def test_deblend_fields_appends_the_weighted_columns():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch
    from debvader_amd.measure import measurement as ms

    sig = inspect.signature(DeblendFieldBatch.deblend_fields).parameters
    assert sig["fit_weights"].default is None and sig["fit_weights"].kind is inspect.Parameter.KEYWORD_ONLY
    net, b = _batch()
    W = np.random.default_rng(5).uniform(0.5, 2.0, size=(4, F, F, NB))
    want = np.dtype(DeblendFieldBatch.ON_DEVICE_COLUMNS + DeblendFieldBatch.measure_columns(NB) +
                    DeblendFieldBatch.fit_flux_weighted_columns(NB))
    for rf in (True, False):
        res = b.deblend_fields(DIST, on_device=True, measure=True, fit_flux=True, fit_weights=W, return_fields=rf)
        (call,) = _engine_calls(net)[-1:]
        assert call[0] == "infer_fields_measure_fit_weighted" and call[2] is rf and call[3] is not None       # places: always
        assert call[4].dtype == np.float64 and np.array_equal(call[4], W)
        assert [len(r) for r in res] == [2, 0, 1, 0] and all(r.dtype == want for r in res)
        f, c = stub_fit_flux_weighted(3, NB), stub_catalogue(3, NB)
        cat = ms.fit_flux_records(*(f[k] for k in KEYS), c["flux"], fit_chi2=f["fit_chi2"], fit_npix=f["fit_npix"])
        for i, (m, k) in enumerate([(0, 0), (0, 1), (2, 0)]):
            for n in cat.dtype.names:
                assert np.array_equal(res[m][n][k], cat[n][i], equal_nan=True), n
        assert np.array_equal(res[0]["fit_scale_err"][0], np.sqrt(f["fit_var"][0]))
    # without fit_weights the call and the columns are those of before
    res = b.deblend_fields(DIST, on_device=True, measure=True, fit_flux=True)
    assert _engine_calls(net)[-1][0] == "infer_fields_measure_fit" and "fit_chi2" not in res[0].dtype.names
    assert np.isnan(res[0]["fit_scale_err"]).all()


def test_deblend_fields_refuses_fit_weights_combinations():
    net, b = _batch()
    W = np.ones((4, F, F, NB))
    on = dict(on_device=True, measure=True)
    for kw, match in ((dict(fit_weights=W, **on), "fit_weights needs fit_flux=True"),
                      (dict(fit_weights=W), "fit_weights needs fit_flux=True"),
                      (dict(fit_weights=W, fit_flux=True), "fit_flux=True needs measure=True and on_device=True"),
                      (dict(fit_weights=W, fit_flux=True, measure=True), "fit_flux=True needs measure=True and on_device=True"),
                      (dict(fit_weights=W, fit_flux=True, on_device=True), "fit_flux=True needs measure=True and on_device=True"),
                      # beside fit_flux it changes no other refusal
                      (dict(fit_weights=W, fit_flux=True, psf=np.ones((21, 21)), **on), "fit_flux=True cannot be combined with psf"),
                      (dict(fit_weights=W, fit_flux=True, apertures=(3.0,), **on), "fit_flux=True cannot be combined with apertures"),
                      (dict(fit_weights=W, fit_flux=True, apertures=(3.0,), aperture_data=True, **on),
                       "fit_flux=True cannot be combined with apertures"),
                      (dict(fit_weights=W, fit_flux=True, blendedness=True, **on), "fit_flux=True cannot be combined with blendedness"),
                      (dict(fit_weights=W, fit_flux=True, measure_samples=4, **on),
                       "fit_flux=True cannot be combined with measure_samples"),
                      (dict(fit_weights=W, fit_flux=True, optimise_positions=True, **on),
                       "fit_flux=True cannot be combined with optimise_positions"),
                      (dict(fit_weights=W, fit_flux=True, epistemic_uncertainty_estimation=True, **on),
                       "fit_flux=True cannot be combined with epistemic_uncertainty_estimation"),
                      # every other extra without fit_flux: fit_weights is refused first or last, never accepted
                      (dict(fit_weights=W, psf=np.ones((21, 21)), **on), "fit_weights needs fit_flux=True"),
                      (dict(fit_weights=W, apertures=(3.0,), **on), "fit_weights needs fit_flux=True"),
                      (dict(fit_weights=W, blendedness=True, **on), "fit_weights needs fit_flux=True"),
                      (dict(fit_weights=W, measure_samples=4, **on), "fit_weights needs fit_flux=True"),
                      # the noise is given once
                      (dict(fit_weights=W, fit_flux=True, sky_sigma=np.ones(NB), **on), "weights already carry the noise"),
                      # the shape of the fields, before any GPU work
                      (dict(fit_weights=W[:3], fit_flux=True, **on), "expected weight fields of the shape of the data fields"),
                      (dict(fit_weights=W[..., :3], fit_flux=True, **on), "expected weight fields of the shape of the data fields"),
                      (dict(fit_weights=W[0], fit_flux=True, **on), "expected weight fields of the shape of the data fields")):
        with pytest.raises(ValueError, match=match):
            b.deblend_fields(DIST, **kw)
    assert not _engine_calls(net) and net._core.seed_counter == 7


def test_engine_wrappers_refuse_before_the_library():
    from debvader_amd import engine as E

    P, pl, D = np.zeros((2, 31, 31, 3), np.float32), np.zeros((2, 2), np.int32), np.zeros((1, 40, 40, 3))
    call = lambda *a, **kw: E.Context.scene_fit_flux(object(), *a, **kw)     # noqa: E731
    for bad in (np.zeros((1, 40, 40, 2)), np.zeros((2, 40, 40, 3)), np.zeros((1, 40, 41, 3)), np.zeros((40, 3)), 2.0):
        with pytest.raises(ValueError, match="expected weight fields of the shape of the data fields"):
            call(P, pl, D, weight_fields=bad)
    with pytest.raises(ValueError, match="min_pivot"):
        call(P, pl, D, weight_fields=np.ones_like(D), min_pivot=0.0)
    fields = np.zeros((2, 81, 81, 6))
    for kw, match in ((dict(places=None, w=fields), "places are needed"),
                      (dict(places=None, w=fields, return_fields=False), "places are needed"),
                      (dict(places=[[0, 0]], w=fields[:1]), "expected weight fields of the shape of the data fields"),
                      (dict(places=[[0, 0]], w=fields[..., :5]), "expected weight fields of the shape of the data fields"),
                      (dict(places=[[0, 0]], w=fields, min_pivot=2.0), "min_pivot"),
                      (dict(places=[[0, 0]], w=fields, band=7), "band")):
        places, w = kw.pop("places"), kw.pop("w")
        with pytest.raises(ValueError, match=match):
            E.Engine.infer_fields_measure_fit_weighted(object(), fields, [[0, 0]], [0, 1, 1], places, w, **kw)
    out, ptrs = E._fit_flux_out(4, 6, True)
    assert list(out) == list(E.FIT_FLUX_WEIGHTED_KEYS) == list(WKEYS) and len(ptrs) == 7 and not any(p is None for p in ptrs)
    assert out["fit_chi2"].shape == out["fit_npix"].shape == (4, 6) and out["fit_npix"].dtype == np.int32
    assert list(E._fit_flux_out(4, 6)[0]) == list(KEYS)
    # an empty call returns without the library; a single weight field is one field
    empty = call(P[:0], pl[:0], D, weight_fields=np.ones((40, 40, 3)))
    assert empty["fit_chi2"].shape == (0, 3) and empty["fit_npix"].dtype == np.int32 and list(empty) == list(WKEYS)
    p = inspect.signature(E.Context.scene_fit_flux).parameters
    assert list(p)[-1] == "weight_fields" and p["weight_fields"].default is None
    assert "weight_field" in inspect.signature(E.Engine.infer_cutouts_measure_fit_weighted).parameters


def test_header_binding_and_library_agree_on_the_weighted_entry_points():
    from debvader_amd import _lib

    header = open(os.path.join(ROOT, "include", "debvader_hip.h")).read()
    ctype = {"dv_model*": C.c_void_p, "dv_ctx*": C.c_void_p, "double*": C.POINTER(C.c_double), "float*": C.POINTER(C.c_float),
             "int32_t*": C.POINTER(C.c_int32), "int64_t*": C.POINTER(C.c_int64), "int32_t": C.c_int32, "int64_t": C.c_int64,
             "uint64_t": C.c_uint64, "double": C.c_double, "dv_measure_params*": C.POINTER(_lib.DvMeasureParams),
             "dv_fit_flux_params*": C.POINTER(_lib.DvFitFluxParams)}
    for name, nargs in (("dv_scene_fit_flux_weighted", 19), ("dv_infer_fields_measure_fit_weighted", 29)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header, re.S)
        assert m, f"{name} is not declared in include/debvader_hip.h"
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)         # bound: the library exports it
        restype, argtypes = _lib.SIGNATURES[name]
        want = [ctype[t] for t in _c_types(m.group(1))]
        assert restype is C.c_int and len(argtypes) == len(want) == nargs
        for i, (a, w) in enumerate(zip(argtypes, want)):
            assert a is w, (name, i, a, w)
        assert getattr(_lib.lib, name).argtypes == argtypes
    # the unweighted calls' arguments with weight_fields behind the data fields / the params, and the two outputs last
    sw, su = _lib.SIGNATURES["dv_scene_fit_flux_weighted"][1], _lib.SIGNATURES["dv_scene_fit_flux"][1]
    assert sw[:8] == su[:8] and sw[8] is C.POINTER(C.c_double) and sw[9:17] == su[8:] and sw[17:] == [C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    pw, pu = _lib.SIGNATURES["dv_infer_fields_measure_fit_weighted"][1], _lib.SIGNATURES["dv_infer_fields_measure_fit"][1]
    assert pw[:21] == pu[:21] and pw[21] is C.POINTER(C.c_double) and pw[22:27] == pu[21:] and pw[27:] == sw[17:]
    # the existing entry points keep their signatures
    assert len(su) == 16 and len(pu) == 26 and len(_lib.SIGNATURES["dv_scene_fit_flux_gram"][1]) == 10
    kernel = open(os.path.join(ROOT, "debvader_amd", "csrc", "fitflux.hip")).read()
    assert "fitflux_chi2_kernel" in kernel and "template <bool WEIGHTED>" in kernel and "getenv" not in kernel
    engine = open(os.path.join(ROOT, "debvader_amd", "csrc", "engine.hip")).read()
    assert "dv_infer_fields_measure_fit_weighted" in engine and "dv_scene_fit_flux_weighted" in engine
