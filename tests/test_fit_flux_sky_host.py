"""The flux fit with a sky background fitted jointly without a GPU: the definition on the numpy
restatement of tests/fit_flux_sky_oracle.py - the bias a sky residual puts into a fit without sky and that the sky term
removes, the invariants of the bordered system, noise realisations against the reported errors - and the host layer
(measurement.fit_sky_records / fit_fluxes_sky, DeblendFieldBatch.deblend_fields(fit_sky=...), the engine wrappers and the
ctypes signatures) over the stand-ins of tests/stub_fit_flux_sky_engine.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests import fit_flux_oracle as fo
from tests import fit_flux_sky_oracle as fs
from tests.stub_fit_flux_sky_engine import CS, KEYS, NB, SKY_KEYS, WKEYS, Net, OracleContext, stub_sky
from tests.stub_fit_flux_weighted_engine import stub_fit_flux_weighted
from tests.stub_measure_engine import stub_catalogue
from tests.test_fit_flux_host import CS31, F64, M1, M2, O1, O2, _c_types, _paste, _stamp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pair_sky():
    """the issue's pair: two noise-free Gaussians 6 px apart, cs = 31, F = 64; D = P1 + P2 without sky"""
    P = np.stack([_stamp(M1, O1), _stamp(M2, O2, amp=1.7)])
    places = np.array([[16, 14], [16, 20]])
    return P, places, _paste(F64, P, places)


def test_a_sky_residual_biases_the_fit_without_sky_and_the_sky_term_removes_it():
    P, places, D0 = _pair_sky()
    D = D0 + 0.05
    plain, _ = fo.fit_flux(P, places, [0, 2], D[None])
    assert (np.abs(plain["fit_scale"] - 1.0).max(axis=1) > 0.02).any(), plain["fit_scale"]      # the reason the feature exists
    got, _ = fs.fit_flux_sky(P, places, [0, 2], D[None], 0)
    assert (got["fit_status"] == 0).all() and (got["sky_status"] == 0).all()
    assert np.abs(got["fit_scale"] - 1.0).max() < 1e-10 and np.abs(got["sky_coef"] - 0.05).max() < 1e-10
    assert (got["sky_npix"] == F64 * F64).all() and got["sky_npix"].dtype == np.int64
    # a plane on top: order 1 recovers its three coefficients, in every band
    B = fs.basis(F64, 3)
    s = np.array([0.05, 0.02, -0.03])
    D = D0 + (B @ s)[:, :, None]
    got, _ = fs.fit_flux_sky(P, places, [0, 2], D[None], 1)
    assert (got["fit_status"] == 0).all() and (got["sky_status"] == 0).all()
    assert np.abs(got["fit_scale"] - 1.0).max() < 1e-10 and np.abs(got["sky_coef"] - s).max() < 1e-10
    # order 0 on the plane is biased again: the order matters
    flat, _ = fs.fit_flux_sky(P, places, [0, 2], D[None], 0)
    assert np.abs(flat["fit_scale"] - 1.0).max() > 1e-4


def test_the_basis_has_an_integer_numerator_and_one_division():
    for F in (1, 2, 64, 97):
        B = fs.basis(F, 3)
        assert (B[:, :, 0] == 1.0).all()
        for r in (0, F // 2, F - 1):
            assert B[r, 0, 1] == np.float64(2 * r - F + 1) / np.float64(F) and B[0, r, 2] == B[r, 0, 1]
        assert np.array_equal(B[:, :, 1], -B[::-1, :, 1])                  # antisymmetric about the field centre, exactly


def test_without_coupling_the_galaxy_rows_are_the_fit_without_sky():
    P, places, D0 = _pair_sky()
    D = D0 + 0.05 + np.random.default_rng(1).normal(0.0, 0.05, size=D0.shape)
    want, _ = fo.fit_flux(P, places, [0, 2], D[None])
    for order in (0, 1):
        got, _ = fs.fit_flux_sky(P, places, [0, 2], D[None], order, zero_coupling=True)
        for k in KEYS:
            assert np.array_equal(got[k], want[k], equal_nan=True), (order, k)
        # ... and the sky is then the mean (the plane) of D alone
        assert np.abs(got["sky_coef"][0, :, 0] - D.mean(axis=(0, 1))).max() < 1e-13


def test_the_galaxies_keep_status_gram_and_proj_on_the_71_galaxy_scene():
    from tests.test_gpu_fit_flux import _scene

    _, P, places, fp, D = _scene(31, 3, 64)
    want, _ = fo.fit_flux(P, places, fp, D)
    assert (want["fit_status"] == 5).any() and (want["fit_status"] == 4).any()         # the scene has both
    for order in (0, 1):
        got, fields = fs.fit_flux_sky(P, places, fp, D, order)
        for k in ("fit_status", "fit_gram", "fit_proj"):
            assert np.array_equal(got[k], want[k]), (order, k)
        assert (got["sky_status"] == 0).all()
        assert max(fs.scaled_condition(s["full"], s["kept"]) for f in fields for s in f["bands"]) < 100.0


def test_a_lone_galaxy_has_the_closed_form():
    P = _stamp(M1, O1)[None]
    places = np.array([[20, 11]])
    D = _paste(F64, P, places, [1.3]) + 0.07 + np.random.default_rng(2).normal(0.0, 0.02, size=(F64, F64, 3))
    got, fields = fs.fit_flux_sky(P, places, [0, 1], D[None], 0)
    for b in range(3):
        A, rhs = fields[0]["A"][b], fields[0]["rhs"][:, b]
        G, E, K, h, c = A[0, 0], A[1, 0], A[1, 1], rhs[0], rhs[1]
        det = G * K - E * E
        assert abs(got["fit_scale"][0, b] - (K * h - E * c) / det) <= 1e-12 * abs(got["fit_scale"][0, b])
        assert abs(got["fit_var"][0, b] - K / det) <= 1e-12 * got["fit_var"][0, b]
        assert abs(got["sky_cov"][0, b, 0, 0] - G / det) <= 1e-12 * got["sky_cov"][0, b, 0, 0]
        assert got["fit_var"][0, b] > 1.0 / G                               # the covariance with the sky only adds variance


def test_an_empty_field_gets_the_mean_of_its_pixels():
    D = np.random.default_rng(3).normal(2.0, 1.0, size=(1, F64, F64, 3))
    got, _ = fs.fit_flux_sky(np.zeros((0, CS31, CS31, 3), np.float32), np.zeros((0, 2), np.int64), [0, 0], D, 0)
    assert got["fit_scale"].shape == (0, 3) and (got["sky_status"] == 0).all()
    assert np.abs(got["sky_coef"][0, :, 0] - D[0].mean(axis=(0, 1))).max() <= 1e-14 * np.abs(D[0].mean(axis=(0, 1))).max()
    assert np.abs(got["sky_cov"][0, :, 0, 0] * F64 * F64 - 1.0).max() < 1e-14
    W = np.random.default_rng(4).uniform(0.5, 2.0, size=D.shape)
    got, _ = fs.fit_flux_sky(np.zeros((0, CS31, CS31, 3), np.float32), np.zeros((0, 2), np.int64), [0, 0], D, 0, W)
    mean = (W * D).sum(axis=(1, 2)) / W.sum(axis=(1, 2))
    assert np.abs(got["sky_coef"][0, :, 0] - mean[0]).max() <= 1e-13 * np.abs(mean).max()


def test_a_wholly_masked_field_is_ineligible():
    P, places, D0 = _pair_sky()
    W = np.ones_like(D0)
    W[:, :, 1] = 0.0
    D = D0.copy()
    D[:, :, 1] = np.nan
    for order in (0, 1):
        got, _ = fs.fit_flux_sky(P, places, [0, 2], D[None], order, W[None])
        assert (got["sky_status"][0, 1] == 4).all() and (got["sky_status"][0, [0, 2]] == 0).all()
        assert np.isnan(got["sky_coef"][0, 1]).all() and np.isnan(got["sky_cov"][0, 1]).all()
        assert np.isfinite(got["sky_coef"][0, [0, 2]]).all() and np.isfinite(got["sky_cov"][0, [0, 2]]).all()
        assert (got["fit_status"][:, 1] == 4).all() and got["sky_npix"][0, 1] == 0 and (got["fit_npix"][:, 1] == 0).all()
        assert np.isnan(got["fit_chi2"][:, 1]).all() and np.isfinite(got["fit_chi2"][:, [0, 2]]).all()


def test_a_plane_term_without_leverage_is_dropped_at_exactly_zero():
    P, places, D0 = _pair_sky()
    D = D0 + 0.05
    W = np.zeros_like(D)
    W[30] = 1.0                                                             # the only counting pixels: one row - B_1 is a constant there
    got, fields = fs.fit_flux_sky(P, places, [0, 2], D[None], 1, W[None])
    assert np.array_equal(got["sky_status"][0], np.tile([0, 5, 0], (3, 1))), got["sky_status"]    # the pattern, first
    assert (got["sky_coef"][0, :, 1] == 0.0).all() and not np.signbit(got["sky_coef"][0, :, 1]).any()
    assert np.isnan(got["sky_cov"][0, :, 1, :]).all() and np.isnan(got["sky_cov"][0, :, :, 1]).all()
    assert np.isfinite(got["sky_cov"][0][:, [0, 2]][:, :, [0, 2]]).all()
    # the dropped term is never applied and nothing is subtracted for it: the kept system is the one without it
    keep = [0, 1, 2, 4]
    for b in range(3):
        A = fields[0]["bands"][b]["full"][np.ix_(keep, keep)]
        x = np.linalg.solve(A, fields[0]["rhs"][keep, b])
        assert np.abs(x[:2] - got["fit_scale"][:, b]).max() < 1e-9 and np.abs(x[2:] - got["sky_coef"][0, b, [0, 2]]).max() < 1e-9
    assert (got["sky_npix"] == F64).all()


def test_a_dropped_galaxy_keeps_amplitude_one_in_the_sky_rows_too():
    P, places, D0 = _pair_sky()
    P = np.concatenate([P, P[:1]])                                          # an exact duplicate of galaxy 0, behind the pair
    places = np.concatenate([places, places[:1]])
    D = _paste(F64, P, places) + 0.05                                       # every model at amplitude 1, the duplicate included
    got, _ = fs.fit_flux_sky(P, places, [0, 3], D[None], 0)
    assert np.array_equal(got["fit_status"], np.tile([[0], [0], [5]], (1, 3)))
    assert (got["fit_scale"][2] == 1.0).all() and np.isnan(got["fit_var"][2]).all()
    assert np.abs(got["fit_scale"][:2] - 1.0).max() < 1e-10 and np.abs(got["sky_coef"] - 0.05).max() < 1e-10


def test_noise_realisations_agree_with_the_reported_errors():
    P, places, D0 = _pair_sky()
    rng = np.random.default_rng(11)
    sigma, n = 0.05, 400
    a, s = np.zeros((n, 2, 3)), np.zeros((n, 3))
    for k in range(n):
        got, _ = fs.fit_flux_sky(P, places, [0, 2], (D0 + 0.05 + rng.normal(0.0, sigma, size=D0.shape))[None], 0)
        a[k], s[k] = got["fit_scale"], got["sky_coef"][0, :, 0]
    err_a, err_s = sigma * np.sqrt(got["fit_var"]), sigma * np.sqrt(got["sky_cov"][0, :, 0, 0])     # (the same in every realisation)
    assert np.abs(a.std(axis=0, ddof=1) / err_a - 1.0).max() < 0.15 and np.abs(s.std(axis=0, ddof=1) / err_s - 1.0).max() < 0.15
    assert (np.abs(a.mean(axis=0) - 1.0) < 4.0 * err_a / np.sqrt(n)).all()
    assert (np.abs(s.mean(axis=0) - 0.05) < 4.0 * err_s / np.sqrt(n)).all()


# ---- the host layer ----------------------------------------------------------------------------------------------------------

def test_fit_sky_records_derive_the_background_under_every_galaxy():
    from debvader_amd.measure import measurement as ms

    assert ms.fit_sky_dtype(NB) == [("fit_sky", "<f8", (NB,)), ("fit_sky_err", "<f8", (NB,))]
    F, M = 81, 4
    places = np.array([[10, 20], [40, 3], [0, 0], [25, 25], [-5, 60]])
    fp = [0, 2, 2, 4, 5]
    field = np.array([0, 0, 2, 2, 3])
    for q in (1, 3):
        sky = stub_sky(M, NB, q, F)
        sigma = np.arange(1, M * NB + 1, dtype=np.float64).reshape(M, NB)
        rec = ms.fit_sky_records(sky["sky_coef"], sky["sky_cov"], sky["sky_status"], places, CS, F, field_ptr=fp, sky_sigma=sigma)
        assert rec.dtype == np.dtype(ms.fit_sky_dtype(NB)) and len(rec) == 5
        for i, m in enumerate(field):
            r, c = places[i] + CS // 2
            b = np.array([1.0, (2 * r - F + 1) / F, (2 * c - F + 1) / F][:q])
            for band in range(NB):
                coef, cov, st = sky["sky_coef"][m, band], sky["sky_cov"][m, band], sky["sky_status"][m, band]
                kept = st == 0
                want = float(coef @ b)
                want_err = float(np.sqrt(b[kept] @ cov[np.ix_(kept, kept)] @ b[kept])) * sigma[m, band]
                assert np.isclose(rec["fit_sky"][i, band], want, rtol=1e-14, atol=0.0)
                assert np.isclose(rec["fit_sky_err"][i, band], want_err, rtol=1e-13, atol=0.0)
        # without sky_sigma the error is NaN; weighted, it is sqrt(b^T cov b) as it stands, and sky_sigma is refused
        assert np.isnan(ms.fit_sky_records(sky["sky_coef"], sky["sky_cov"], sky["sky_status"], places, CS, F,
                                           field_ptr=fp)["fit_sky_err"]).all()
        w = ms.fit_sky_records(sky["sky_coef"], sky["sky_cov"], sky["sky_status"], places, CS, F, field_ptr=fp, weighted=True)
        assert np.allclose(w["fit_sky_err"] * sigma[field], rec["fit_sky_err"], rtol=1e-14, atol=0.0)
        with pytest.raises(ValueError, match="weights already carry the noise"):
            ms.fit_sky_records(sky["sky_coef"], sky["sky_cov"], sky["sky_status"], places, CS, F, field_ptr=fp, sky_sigma=sigma,
                               weighted=True)
    # the NaN rules: a field without a counting pixel is NaN in both columns of that band; a dropped term adds nothing
    sky = stub_sky(M, NB, 3, F)
    rec = ms.fit_sky_records(sky["sky_coef"], sky["sky_cov"], sky["sky_status"], [[3, 3]] * 3, CS, F, field_ptr=[0, 0, 1, 3, 3],
                             weighted=True)
    assert np.isnan(rec["fit_sky"][0, -1]) and np.isnan(rec["fit_sky_err"][0, -1]) and np.isfinite(rec["fit_sky"][0, :-1]).all()
    assert np.isfinite(rec["fit_sky"][1:]).all() and np.isfinite(rec["fit_sky_err"][1:]).all()
    for bad, match in ((dict(field_ptr=[0, 1, 3]), "field_ptr must have"), (dict(field_ptr=[0, 0, 1, 2, 2]), "field_ptr must have")):
        with pytest.raises(ValueError, match=match):
            ms.fit_sky_records(sky["sky_coef"], sky["sky_cov"], sky["sky_status"], [[3, 3]] * 3, CS, F, **bad)
    with pytest.raises(ValueError, match="expected sky_coef"):
        ms.fit_sky_records(np.zeros((4, NB, 2)), np.zeros((4, NB, 2, 2)), np.zeros((4, NB, 2)), [[3, 3]], CS, F)


def test_fit_fluxes_sky_returns_the_catalogue_and_the_field_arrays():
    from debvader_amd.measure import measurement as ms

    P, places, D0 = _pair_sky()
    D = D0 + 0.05
    ctx = OracleContext()
    for W in (None, np.full_like(D, 4.0)):
        for order, q in ((0, 1), (1, 3)):
            cat, sky = ms.fit_fluxes_sky(P, places, D, sky_order=order, weight_fields=W, sky_sigma=None if W is not None else
                                         np.full(3, 0.5), ctx=ctx)
            base = ms.fit_flux_dtype(3) if W is None else ms.fit_flux_weighted_dtype(3)
            assert cat.dtype == np.dtype(base + ms.fit_sky_dtype(3)) and len(cat) == 2
            assert list(sky) == list(SKY_KEYS) and sky["sky_coef"].shape == (1, 3, q) and sky["sky_cov"].shape == (1, 3, q, q)
            assert sky["sky_status"].dtype == np.int32 and sky["sky_npix"].dtype == np.int64
            assert ctx.calls[-1]["sky_order"] == order and ctx.calls[-1]["fit_flux_sky"] == 2
            assert np.abs(cat["fit_scale"] - 1.0).max() < 1e-9 and np.abs(cat["fit_sky"] - 0.05).max() < 1e-9
            assert np.abs(cat["flux_fit"] - P.sum(axis=(1, 2), dtype=np.float64)).max() < 1e-6
            want = ms.fit_sky_records(sky["sky_coef"], sky["sky_cov"], sky["sky_status"], places, CS31, F64,
                                      sky_sigma=None if W is not None else np.full(3, 0.5), weighted=W is not None)
            assert np.array_equal(cat["fit_sky_err"], want["fit_sky_err"]) and (cat["fit_sky_err"] > 0).all()
            assert np.array_equal(cat["fit_scale_err"], np.sqrt(cat["fit_var"]) * (0.5 if W is None else 1.0))
    # a constant weight 1 / sigma^2 is the unweighted fit with sky_sigma = sigma
    plain, _ = ms.fit_fluxes_sky(P, places, D, sky_order=1, sky_sigma=np.full(3, 0.5), ctx=ctx)
    assert np.allclose(cat["fit_sky_err"], plain["fit_sky_err"], rtol=1e-9, atol=0.0)
    assert np.allclose(cat["fit_scale_err"], plain["fit_scale_err"], rtol=1e-9, atol=0.0)
    # without sky_sigma, unweighted: NaN errors
    cat, _ = ms.fit_fluxes_sky(P, places, D, ctx=ctx)
    assert np.isnan(cat["fit_sky_err"]).all() and np.isnan(cat["fit_scale_err"]).all() and ctx.calls[-1]["sky_order"] == 0
    before = len(ctx.calls)
    for kw, match in ((dict(sky_order=2), "sky_order must be 0"), (dict(sky_order=True), "sky_order must be 0"),
                      (dict(sky_order=-1), "sky_order must be 0"), (dict(sky_order=None), "sky_order must be 0"),
                      (dict(weight_fields=np.ones_like(D), sky_sigma=np.ones(3)), "weights already carry the noise"),
                      (dict(weight_fields=np.ones((F64, F64, 2))), "expected weight fields of the shape of the data fields"),
                      (dict(sky_sigma=np.ones(4)), "sky_sigma"),
                      (dict(catalogue=np.recarray((2,), dtype=[("x", "<f8")])), "lacks the column flux")):
        with pytest.raises(ValueError, match=match):
            ms.fit_fluxes_sky(P, places, D, ctx=ctx, **kw)
    assert len(ctx.calls) == before
    # the pinned parameter lists of the calls without sky
    assert list(inspect.signature(ms.fit_fluxes).parameters) == ["stamps_mean", "places", "data_fields", "field_ptr", "catalogue",
                                                                 "sky_sigma", "min_pivot", "ctx"]
    assert list(inspect.signature(ms.fit_fluxes_weighted).parameters) == ["stamps_mean", "places", "data_fields", "weight_fields",
                                                                          "field_ptr", "catalogue", "sky_sigma", "min_pivot", "ctx"]
    assert list(inspect.signature(ms.fit_fluxes_sky).parameters)[:5] == ["stamps_mean", "places", "data_fields", "sky_order",
                                                                         "weight_fields"]


F = 81
DIST = [np.array([[0.0, 0.0], [5.0, -7.0]]), np.zeros((0, 2)), np.array([[100.0, 0.0], [-3.0, 11.0]]), np.array([[0.0, 40.0]])]


def _batch():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch

    net = Net()
    return net, DeblendFieldBatch(net, np.random.default_rng(3).normal(size=(4, F, F, NB)), CS, NB)


def _engine_calls(net):
    return [c for c in net._core.engine.calls if c[0].startswith("infer")]


def test_deblend_fields_appends_the_sky_columns_and_keeps_the_field_arrays():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch
    from debvader_amd.measure import measurement as ms

    sig = inspect.signature(DeblendFieldBatch.deblend_fields).parameters
    assert sig["fit_sky"].default is None and sig["fit_sky"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(sig)[-2:] == ["fit_sky", "optimise_positions"]
    assert DeblendFieldBatch.fit_sky_columns(NB) == ms.fit_sky_dtype(NB)
    net, b = _batch()
    assert b.sky_fit is None
    W = np.random.default_rng(5).uniform(0.5, 2.0, size=(4, F, F, NB))
    places = (int((F - CS) / 2) + np.array([[0, 0], [5, -7], [-3, 11]])).astype(np.int64)      # the three galaxies that pass the border cut
    for weights in (None, W):
        fit_cols = DeblendFieldBatch.fit_flux_columns(NB) if weights is None else DeblendFieldBatch.fit_flux_weighted_columns(NB)
        want = np.dtype(DeblendFieldBatch.ON_DEVICE_COLUMNS + DeblendFieldBatch.measure_columns(NB) + fit_cols +
                        DeblendFieldBatch.fit_sky_columns(NB))
        for order, q in ((0, 1), (1, 3)):
            for rf in (True, False):
                sky_sigma = None if weights is not None else np.full(NB, 0.3)
                res = b.deblend_fields(DIST, on_device=True, measure=True, fit_flux=True, fit_sky=order, fit_weights=weights,
                                       sky_sigma=sky_sigma, return_fields=rf)
                (call,) = _engine_calls(net)[-1:]
                assert call[0] == "infer_fields_measure_fit_sky" and call[2] is rf and np.array_equal(call[3], places)
                assert call[4] == order and (call[5] is None if weights is None else np.array_equal(call[5], W))
                assert [len(r) for r in res] == [2, 0, 1, 0] and all(r.dtype == want for r in res)
                f, c, sky = stub_fit_flux_weighted(3, NB), stub_catalogue(3, NB), stub_sky(4, NB, q, F)
                if weights is None:
                    cat = ms.fit_flux_records(*(f[k] for k in KEYS), c["flux"], sky_sigma=sky_sigma, field_ptr=[0, 2, 2, 3, 3])
                else:
                    cat = ms.fit_flux_records(*(f[k] for k in KEYS), c["flux"], fit_chi2=f["fit_chi2"], fit_npix=f["fit_npix"])
                srec = ms.fit_sky_records(sky["sky_coef"], sky["sky_cov"], sky["sky_status"], places, CS, F,
                                          field_ptr=[0, 2, 2, 3, 3], sky_sigma=sky_sigma, weighted=weights is not None)
                for i, (m, k) in enumerate([(0, 0), (0, 1), (2, 0)]):
                    for part in (cat, srec):
                        for n in part.dtype.names:
                            assert np.array_equal(res[m][n][k], part[n][i], equal_nan=True), n
                assert list(b.sky_fit) == list(SKY_KEYS)
                for k in SKY_KEYS:
                    assert np.array_equal(b.sky_fit[k], sky[k], equal_nan=True) and b.sky_fit[k].shape[0] == 4
    # without fit_sky the calls, the columns and the attribute are those of before
    res = b.deblend_fields(DIST, on_device=True, measure=True, fit_flux=True)
    assert _engine_calls(net)[-1][0] == "infer_fields_measure_fit" and "fit_sky" not in res[0].dtype.names and b.sky_fit is None
    res = b.deblend_fields(DIST, on_device=True, measure=True, fit_flux=True, fit_weights=W)
    assert _engine_calls(net)[-1][0] == "infer_fields_measure_fit_weighted" and "fit_sky" not in res[0].dtype.names


def test_deblend_fields_refuses_fit_sky_combinations():
    net, b = _batch()
    W = np.ones((4, F, F, NB))
    on = dict(on_device=True, measure=True)
    for kw, match in ((dict(fit_sky=0, **on), "fit_sky needs fit_flux=True"),
                      (dict(fit_sky=1), "fit_sky needs fit_flux=True"),
                      (dict(fit_sky=0, fit_weights=W, **on), "needs fit_flux=True"),
                      (dict(fit_sky=0, fit_flux=True), "fit_flux=True needs measure=True and on_device=True"),
                      (dict(fit_sky=0, fit_flux=True, measure=True), "fit_flux=True needs measure=True and on_device=True"),
                      (dict(fit_sky=0, fit_flux=True, on_device=True), "fit_flux=True needs measure=True and on_device=True"),
                      # the order, before any GPU work
                      (dict(fit_sky=2, fit_flux=True, **on), "sky_order must be 0"),
                      (dict(fit_sky=-1, fit_flux=True, **on), "sky_order must be 0"),
                      (dict(fit_sky=True, fit_flux=True, **on), "sky_order must be 0"),
                      (dict(fit_sky=0.5, fit_flux=True, **on), "sky_order must be 0"),
                      # beside every non-fit extra it is still refused
                      (dict(fit_sky=1, fit_flux=True, psf=np.ones((21, 21)), **on), "fit_flux=True cannot be combined with psf"),
                      (dict(fit_sky=1, fit_flux=True, apertures=(3.0,), **on), "fit_flux=True cannot be combined with apertures"),
                      (dict(fit_sky=1, fit_flux=True, apertures=(3.0,), aperture_data=True, **on),
                       "fit_flux=True cannot be combined with apertures"),
                      (dict(fit_sky=1, fit_flux=True, blendedness=True, **on), "fit_flux=True cannot be combined with blendedness"),
                      (dict(fit_sky=1, fit_flux=True, measure_samples=4, **on), "fit_flux=True cannot be combined with measure_samples"),
                      (dict(fit_sky=1, fit_flux=True, optimise_positions=True, **on),
                       "fit_flux=True cannot be combined with optimise_positions"),
                      (dict(fit_sky=1, fit_flux=True, epistemic_uncertainty_estimation=True, **on),
                       "fit_flux=True cannot be combined with epistemic_uncertainty_estimation"),
                      (dict(fit_sky=0, psf=np.ones((21, 21)), **on), "fit_sky needs fit_flux=True"),
                      (dict(fit_sky=0, apertures=(3.0,), **on), "fit_sky needs fit_flux=True"),
                      (dict(fit_sky=0, blendedness=True, **on), "fit_sky needs fit_flux=True"),
                      (dict(fit_sky=0, measure_samples=4, **on), "fit_sky needs fit_flux=True"),
                      # the noise is given once
                      (dict(fit_sky=0, fit_weights=W, fit_flux=True, sky_sigma=np.ones(NB), **on), "weights already carry the noise"),
                      (dict(fit_sky=0, fit_weights=W[:3], fit_flux=True, **on), "expected weight fields of the shape of the data fields")):
        with pytest.raises(ValueError, match=match):
            b.deblend_fields(DIST, **kw)
    assert not _engine_calls(net) and net._core.seed_counter == 7


def test_engine_wrappers_refuse_before_the_library():
    from debvader_amd import engine as E

    assert E.sky_terms(0) == 1 and E.sky_terms(1) == 3 and E.sky_terms(np.int64(1)) == 3
    P, pl, D = np.zeros((2, 31, 31, 3), np.float32), np.zeros((2, 2), np.int32), np.zeros((1, 40, 40, 3))
    call = lambda *a, **kw: E.Context.scene_fit_flux_sky(object(), *a, **kw)     # noqa: E731
    for kw, match in ((dict(sky_order=2), "sky_order must be 0"), (dict(sky_order=None), "sky_order must be 0"),
                      (dict(weight_fields=np.zeros((1, 40, 40, 2))), "expected weight fields of the shape of the data fields"),
                      (dict(min_pivot=0.0), "min_pivot"), (dict(scratch_bytes=0), "scratch_bytes"),
                      (dict(field_ptr=[0, 1]), "field_ptr")):
        with pytest.raises(ValueError, match=match):
            call(P, pl, D, **kw)
    with pytest.raises(ValueError, match="expected data fields"):
        call(P, pl, D[0])
    with pytest.raises(ValueError, match="expected places"):
        call(P, pl[:1], D)
    gram = lambda *a, **kw: E.Context.scene_fit_flux_sky_gram(object(), *a, **kw)     # noqa: E731
    with pytest.raises(ValueError, match="sky_order must be 0"):
        gram(P, pl, D[0], sky_order=3)
    with pytest.raises(ValueError, match="expected one data field"):
        gram(P, pl, D)
    fields = np.zeros((2, 81, 81, 6))
    for kw, match in ((dict(places=None), "places are needed"), (dict(places=None, return_fields=False), "places are needed"),
                      (dict(places=[[0, 0]], sky_order=2), "sky_order must be 0"),
                      (dict(places=[[0, 0]], weight_fields=fields[:1]), "expected weight fields of the shape of the data fields"),
                      (dict(places=[[0, 0]], min_pivot=2.0), "min_pivot"), (dict(places=[[0, 0]], band=7), "band")):
        places = kw.pop("places")
        with pytest.raises(ValueError, match=match):
            E.Engine.infer_fields_measure_fit_sky(object(), fields, [[0, 0]], [0, 1, 1], places, **kw)
    out, ptrs = E._fit_sky_out(4, 6, 3)
    assert list(out) == list(E.FIT_SKY_KEYS) == list(SKY_KEYS) and len(ptrs) == 4
    assert out["sky_coef"].shape == (4, 6, 3) and out["sky_cov"].shape == (4, 6, 3, 3) and out["sky_status"].dtype == np.int32
    assert out["sky_npix"].shape == (4, 6) and out["sky_npix"].dtype == np.int64
    # a call without fields returns without the library
    empty = call(P[:0], pl[:0], D[:0], field_ptr=[0])
    assert list(empty) == list(KEYS + SKY_KEYS) and empty["sky_coef"].shape == (0, 3, 1)
    assert list(call(P[:0], pl[:0], D[:0], field_ptr=[0], weight_fields=D[:0], sky_order=1)) == list(WKEYS + SKY_KEYS)
    assert "weight_field" in inspect.signature(E.Engine.infer_cutouts_measure_fit_sky).parameters
    # the calls without sky keep their parameter lists
    p = inspect.signature(E.Context.scene_fit_flux).parameters
    assert list(p)[-1] == "weight_fields" and "sky_order" not in p


def test_header_binding_and_library_agree_on_the_sky_entry_points():
    from debvader_amd import _lib

    header = open(os.path.join(ROOT, "include", "debvader_hip.h")).read()
    ctype = {"dv_model*": C.c_void_p, "dv_ctx*": C.c_void_p, "double*": C.POINTER(C.c_double), "float*": C.POINTER(C.c_float),
             "int32_t*": C.POINTER(C.c_int32), "int64_t*": C.POINTER(C.c_int64), "int32_t": C.c_int32, "int64_t": C.c_int64,
             "uint64_t": C.c_uint64, "double": C.c_double, "dv_measure_params*": C.POINTER(_lib.DvMeasureParams),
             "dv_fit_flux_params*": C.POINTER(_lib.DvFitFluxParams)}
    for name, nargs in (("dv_scene_fit_flux_sky", 24), ("dv_infer_fields_measure_fit_sky", 34), ("dv_scene_fit_flux_sky_gram", 12)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header, re.S)
        assert m, f"{name} is not declared in include/debvader_hip.h"
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)         # bound: the library exports it
        restype, argtypes = _lib.SIGNATURES[name]
        want = [ctype[t] for t in _c_types(m.group(1))]
        assert restype is C.c_int and len(argtypes) == len(want) == nargs
        for i, (a, w) in enumerate(zip(argtypes, want)):
            assert a is w, (name, i, a, w)
        assert getattr(_lib.lib, name).argtypes == argtypes
    # the weighted calls' arguments, sky_order behind the params (the weights), and the four sky outputs last
    sky_out = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    ss, sw = _lib.SIGNATURES["dv_scene_fit_flux_sky"][1], _lib.SIGNATURES["dv_scene_fit_flux_weighted"][1]
    assert ss[:12] == sw[:12] and ss[12] is C.c_int32 and ss[13:20] == sw[12:] and ss[20:] == sky_out
    ps, pw = _lib.SIGNATURES["dv_infer_fields_measure_fit_sky"][1], _lib.SIGNATURES["dv_infer_fields_measure_fit_weighted"][1]
    assert ps[:22] == pw[:22] and ps[22] is C.c_int32 and ps[23:30] == pw[22:] and ps[30:] == sky_out
    # the existing entry points keep their argument counts, and the parameter struct its two fields
    for name, nargs in (("dv_scene_fit_flux", 16), ("dv_infer_fields_measure_fit", 26), ("dv_scene_fit_flux_gram", 10),
                        ("dv_scene_fit_flux_weighted", 19), ("dv_infer_fields_measure_fit_weighted", 29),
                        ("dv_fit_flux_params_default", 1)):
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    assert [f[0] for f in _lib.DvFitFluxParams._fields_] == ["min_pivot", "scratch_bytes"]
    kernel = open(os.path.join(ROOT, "debvader_amd", "csrc", "fitflux.hip")).read()
    for k in ("fitflux_skysum_kernel", "fitflux_skyreduce_kernel", "fitflux_border_kernel", "#pragma clang fp contract(off)"):
        assert k in kernel, k
    assert "getenv" not in kernel
    engine = open(os.path.join(ROOT, "debvader_amd", "csrc", "engine.hip")).read()
    assert "dv_infer_fields_measure_fit_sky" in engine and "dv_scene_fit_flux_sky" in engine
