"""The simultaneous flux fit without a GPU: the definition on the numpy restatement of
tests/fit_flux_oracle.py - closed forms, the dropping rule, the statuses, the error formula against noise realisations - and the
host layer (measurement.fit_flux_records / fit_fluxes, DeblendFieldBatch.deblend_fields(fit_flux=True), the engine wrappers and
the ctypes signatures) over the stand-ins of tests/stub_fit_flux_engine.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests import fit_flux_oracle as fo
from tests.stub_fit_flux_engine import CS, KEYS, NB, Net, OracleContext, stub_fit_flux
from tests.stub_measure_engine import stub_catalogue

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS31, F64 = 31, 64
BANDS = np.array([0.6, 1.3, 1.0])
M1, O1 = (4.0, 0.8, 3.0), (0.21, -0.33)
M2, O2 = (5.0, -1.0, 3.5), (-0.4, 0.17)


def _stamp(M, off, amp=1.0, cs=CS31):
    """a noise-free elliptical Gaussian in three bands, as the float32 the network would give"""
    return (fo.elliptical_gaussian(cs, M, off, amp)[:, :, None] * BANDS).astype(np.float32)


def _paste(F, stamps, places, amps=None):
    """sum a_i P_i on an F x F field, float64, the stamps clipped at the field edges"""
    nb = stamps[0].shape[2]
    out = np.zeros((F, F, nb))
    for i, (P, (pr, pc)) in enumerate(zip(stamps, places)):
        cs = P.shape[0]
        ra, rz, ca, cz = fo.clip((pr, pc), cs, F)
        if rz > ra and cz > ca:
            out[ra:rz, ca:cz] += (1.0 if amps is None else amps[i]) * P[ra - pr:rz - pr, ca - pc:cz - pc].astype(np.float64)
    return out


def _pair(sep=6, bias=0.9):
    """two galaxies `sep` px apart in one 64-px field, the model of the first `bias` times the truth: (P stamps (2, cs, cs, 3),
    places, D, true amplitudes).  The truth of galaxy 1 is P1 / bias in float64, so D lies exactly in the span of the models."""
    P = np.stack([_stamp(M1, O1), _stamp(M2, O2, amp=1.7)])
    places = np.array([[16, 14], [16, 14 + sep]])
    truth = np.array([1.0 / bias, 1.0])
    return P, places, _paste(F64, P, places, truth), truth


def test_a_biased_neighbour_does_not_bias_the_fitted_fluxes():
    from debvader_amd.measure import measurement as ms

    P, places, D, truth = _pair()
    out, fields = fo.fit_flux(P, places, [0, 2], D[None])
    assert (out["fit_status"] == 0).all()
    assert np.abs(out["fit_scale"] - truth[:, None]).max() < 1e-11
    flux = P.sum(axis=(1, 2), dtype=np.float64)
    rec = ms.fit_flux_records(*(out[k] for k in KEYS), flux)
    true_flux = truth[:, None] * flux
    assert np.abs(rec["flux_fit"] - true_flux).max() < 1e-11 * np.abs(true_flux).max()
    # the aperture-on-data style of correction, sum over the stamp of D - T + P2 with the neighbour at the network's amplitude,
    # keeps a tenth of the neighbour's light under the stamp of galaxy 2; the fit does not
    T = _paste(F64, P, places)
    pr, pc = places[1]
    data_style = (D - T)[pr:pr + CS31, pc:pc + CS31].sum(axis=(0, 1)) + flux[1]
    off = np.abs(data_style - true_flux[1]) / true_flux[1]
    assert (off > 0.02).all() and (np.abs(rec["flux_fit"][1] - true_flux[1]) / true_flux[1] < 1e-11).all()
    # the amplitude with the neighbours ignored is biased by the overlap
    assert (np.abs(rec["fit_scale_alone"] - truth[:, None]) > 1e-3).all()
    for sep in (1, 2, 13):
        P, places, D, truth = _pair(sep)
        out, _ = fo.fit_flux(P, places, [0, 2], D[None])
        assert np.abs(out["fit_scale"] - truth[:, None]).max() < 1e-11, sep


def test_a_lone_galaxy():
    from debvader_amd.measure import measurement as ms

    P = _stamp(M1, O1)[None]
    places = np.array([[20, 11]])
    D = _paste(F64, P, places, [1.3]) + np.random.default_rng(5).normal(0.0, 0.05, size=(F64, F64, 3))
    out, _ = fo.fit_flux(P, places, [0, 1], D[None])
    assert (out["fit_status"] == 0).all() and (out["fit_gram"] > 0).all()
    rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()      # noqa: E731
    assert rel(out["fit_scale"], out["fit_proj"] / out["fit_gram"]) < 1e-15
    assert rel(out["fit_var"], 1.0 / out["fit_gram"]) < 1e-15
    rec = ms.fit_flux_records(*(out[k] for k in KEYS), P.sum(axis=(1, 2), dtype=np.float64))
    assert np.abs(rec["fit_independence"] - 1.0).max() < 1e-15
    assert np.abs(out["fit_scale"] - 1.3).max() < 0.05


def test_two_galaxy_closed_form_of_the_variance():
    for sep in (1, 3, 6):
        P, places, D, _ = _pair(sep)
        out, fields = fo.fit_flux(P, places, [0, 2], D[None])
        for b in range(3):
            G = fields[0]["G"][b]
            det = G[0, 0] * G[1, 1] - G[1, 0] ** 2
            want = np.array([G[1, 1] / det, G[0, 0] / det])
            assert np.abs(out["fit_var"][:, b] - want).max() <= 1e-12 * want.max(), (sep, b)
            assert G[0, 1] == 0.0 and G[1, 0] > 0.0


def test_the_later_of_two_identical_models_is_dropped():
    P1 = _stamp(M1, O1)
    P = np.stack([P1, P1, _stamp(M2, O2)])
    places = np.array([[16, 14], [16, 14], [19, 22]])
    D = _paste(F64, P, places, [1.4, 1.0, 0.8])
    out, fields = fo.fit_flux(P, places, [0, 3], D[None])
    assert out["fit_status"].tolist() == [[0] * 3, [5] * 3, [0] * 3]
    assert (out["fit_scale"][1] == 1.0).all() and np.isnan(out["fit_var"][1]).all()
    # the first is fitted against D - P: the two copies together carry 2.4, the dropped one keeps 1
    assert np.abs(out["fit_scale"][0] - 1.4).max() < 1e-11 and np.abs(out["fit_scale"][2] - 0.8).max() < 1e-11
    two, _ = fo.fit_flux(P[[0, 2]], places[[0, 2]], [0, 2], (D - _paste(F64, P[1:2], places[1:2]))[None])
    assert np.allclose(out["fit_scale"][[0, 2]], two["fit_scale"], rtol=0, atol=1e-12)
    assert np.allclose(out["fit_var"][[0, 2]], two["fit_var"], rtol=1e-12, atol=0)
    assert np.array_equal(out["fit_gram"][1], out["fit_gram"][0]) and np.array_equal(out["fit_proj"][1], out["fit_proj"][0])
    # a wider min_pivot drops a merely similar model too
    P = np.stack([P1, _stamp(M1, (O1[0] + 0.01, O1[1]))])
    D = _paste(F64, P, places[:2])
    assert (fo.fit_flux(P, places[:2], [0, 2], D[None])[0]["fit_status"] == 0).all()
    assert fo.fit_flux(P, places[:2], [0, 2], D[None], min_pivot=1e-2)[0]["fit_status"].tolist() == [[0] * 3, [5] * 3]


def test_a_zero_band_is_ineligible_in_that_band_only():
    P, places, D, truth = _pair()
    P = P.copy()
    P[0, :, :, 1] = 0.0
    out, _ = fo.fit_flux(P, places, [0, 2], D[None])
    assert out["fit_status"].tolist() == [[0, 4, 0], [0, 0, 0]]
    assert np.isnan(out["fit_scale"][0, 1]) and np.isnan(out["fit_var"][0, 1]) and out["fit_gram"][0, 1] == 0.0
    assert np.isfinite(out["fit_scale"][[0, 0, 1, 1, 1], [0, 2, 0, 1, 2]]).all()
    assert np.abs(out["fit_scale"][:, [0, 2]] - truth[:, None]).max() < 1e-11
    # galaxy 2 is alone in band 1
    assert abs(out["fit_var"][1, 1] - 1.0 / out["fit_gram"][1, 1]) < 1e-15 * out["fit_var"][1, 1]


def test_stamps_outside_and_over_a_corner():
    P = np.stack([_stamp(M1, O1), _stamp(M2, O2), _stamp(M1, O1), _stamp(M2, (-4.0, -5.0))])
    places = np.array([[-CS31, 5], [7, F64], [20, 20], [-10, -12]])          # two wholly outside, one inside, one over a corner
    D = _paste(F64, P, places, [1.0, 1.0, 1.2, 0.7])
    out, fields = fo.fit_flux(P, places, [0, 4], D[None])
    assert out["fit_status"].tolist() == [[4] * 3, [4] * 3, [0] * 3, [0] * 3]
    assert (out["fit_gram"][:2] == 0.0).all() and (out["fit_proj"][:2] == 0.0).all()
    assert np.abs(out["fit_scale"][2] - 1.2).max() < 1e-11 and np.abs(out["fit_scale"][3] - 0.7).max() < 1e-11
    clipped = P[3, 10:, 12:, :].astype(np.float64)
    assert np.allclose(out["fit_gram"][3], (clipped * clipped).sum(axis=(0, 1)), rtol=1e-13, atol=0)
    assert (out["fit_gram"][3] < (P[3].astype(np.float64) ** 2).sum(axis=(0, 1))).all()
    assert (fields[0]["G"][:, :, :2] == 0.0).all() and (fields[0]["G"][:, :2, :] == 0.0).all()


def test_the_error_formula_against_noise_realisations():
    """400 realisations of sky noise on the pair at 2 px: the sample standard deviation of fit_scale lies within 15 % of
    sky_sigma sqrt(fit_var) - four standard errors, 1 / sqrt(2 x 399) = 3.5 % each, of a standard deviation estimated from 400
    draws - and its mean within four standard errors of the truth."""
    P, places, D, truth = _pair(2)
    P, D = P[:, :, :, 2:], D[:, :, 2:]
    sky, R = 0.05, 400
    rng = np.random.default_rng(20261)
    base, fields = fo.fit_flux(P, places, [0, 2], D[None])
    G = fields[0]["G"][0]
    P64 = P[:, :, :, 0].astype(np.float64)
    scales = np.zeros((R, 2))
    for k in range(R):
        noise = rng.normal(0.0, sky, size=(F64, F64))
        h = np.array([base["fit_proj"][i, 0] + (P64[i] * noise[pr:pr + CS31, pc:pc + CS31]).sum()
                      for i, (pr, pc) in enumerate(places)])
        s = fo.solve_band(G, h)
        assert (s["status"] == 0).all() and np.array_equal(s["var"], base["fit_var"][:, 0])
        scales[k] = s["scale"]
    want = sky * np.sqrt(base["fit_var"][:, 0])
    got = scales.std(axis=0, ddof=1)
    assert (np.abs(got / want - 1.0) < 0.15).all(), (got, want)
    assert (np.abs(scales.mean(axis=0) - truth) < 4.0 * want / np.sqrt(R)).all()
    # the neighbour costs precision: the joint error exceeds the error with the neighbour held fixed
    assert (base["fit_var"][:, 0] > 1.0 / base["fit_gram"][:, 0]).all()


# ---- the host layer -------------------------------------------------------------------------------------------------------------

def test_fit_flux_records_columns_and_derived_values():
    from debvader_amd.measure import measurement as ms

    n, nb = 7, NB
    f = stub_fit_flux(n, nb)
    flux = stub_catalogue(n, nb)["flux"] - 2.0                   # (some negative: the error takes |flux|)
    names = ("fit_scale", "fit_var", "fit_gram", "fit_proj", "fit_status", "flux_fit", "fit_scale_alone", "fit_independence",
             "fit_scale_err", "flux_fit_err")
    assert tuple(d[0] for d in ms.fit_flux_dtype(nb)) == names
    assert all(d[2] == (nb,) for d in ms.fit_flux_dtype(nb)) and dict((d[0], d[1]) for d in ms.fit_flux_dtype(nb))["fit_status"] == "<i4"
    rec = ms.fit_flux_records(*(f[k] for k in KEYS), flux)
    assert rec.dtype.names == names and len(rec) == n
    for k in KEYS:
        assert np.array_equal(rec[k], f[k], equal_nan=True), k
    assert np.array_equal(rec["flux_fit"], f["fit_scale"] * flux, equal_nan=True)
    ok = f["fit_status"] == 0
    assert np.allclose(rec["fit_scale_alone"][ok], 1.5) and np.allclose(rec["fit_independence"][ok], np.sqrt(0.8))
    assert ((rec["fit_independence"][ok] > 0) & (rec["fit_independence"][ok] <= 1)).all()
    # dropped: the network's amplitude, no variance; ineligible: NaN throughout
    assert f["fit_status"][1, 0] == 5 and rec["flux_fit"][1, 0] == flux[1, 0] and np.isnan(rec["fit_independence"][1, 0])
    assert rec["fit_scale_alone"][1, 0] == 1.5
    assert f["fit_status"][4, -1] == 4
    assert all(np.isnan(rec[k][4, -1]) for k in ("flux_fit", "fit_scale_alone", "fit_independence"))
    assert np.isnan(rec["fit_scale_err"]).all() and np.isnan(rec["flux_fit_err"]).all()       # no sky_sigma
    with pytest.raises(ValueError, match=r"expected flux \(7, 6\)"):
        ms.fit_flux_records(*(f[k] for k in KEYS), flux[:, :3])
    with pytest.raises(ValueError, match=r"expected fit_scale \(N, bands\)"):
        ms.fit_flux_records(f["fit_scale"][0], f["fit_var"], f["fit_gram"], f["fit_proj"], f["fit_status"], flux)


def test_sky_sigma_gives_the_errors():
    from debvader_amd.measure import measurement as ms

    n, nb = 7, NB
    f = stub_fit_flux(n, nb)
    flux = stub_catalogue(n, nb)["flux"] - 2.0
    sky = np.linspace(0.1, 0.6, nb)
    rec = ms.fit_flux_records(*(f[k] for k in KEYS), flux, sky_sigma=sky)
    assert np.array_equal(rec["fit_scale_err"], sky[None, :] * np.sqrt(f["fit_var"]), equal_nan=True)
    assert np.array_equal(rec["flux_fit_err"], sky[None, :] * np.sqrt(f["fit_var"]) * np.abs(flux), equal_nan=True)
    assert (rec["flux_fit_err"][f["fit_status"] == 0] >= 0).all() and np.isnan(rec["fit_scale_err"][1, 0])
    per_field = np.arange(1, 3 * nb + 1, dtype=np.float64).reshape(3, nb)
    fp = [0, 2, 2, 7]
    rec = ms.fit_flux_records(*(f[k] for k in KEYS), flux, sky_sigma=per_field, field_ptr=fp)
    rows = per_field[[0, 0, 2, 2, 2, 2, 2]]
    assert np.array_equal(rec["fit_scale_err"], rows * np.sqrt(f["fit_var"]), equal_nan=True)
    for bad, match in ((np.ones(nb + 1), "sky_sigma must have shape"), (np.ones((2, nb)), "sky_sigma must have shape"),
                       (np.zeros(nb), "finite and positive"), (np.full((3, nb), np.nan), "finite and positive")):
        with pytest.raises(ValueError, match=match):
            ms.fit_flux_records(*(f[k] for k in KEYS), flux, sky_sigma=bad, field_ptr=fp)
    with pytest.raises(ValueError, match="field_ptr must start at 0"):
        ms.fit_flux_records(*(f[k] for k in KEYS), flux, sky_sigma=sky, field_ptr=[0, 3, 6])


def test_fit_fluxes_over_the_restatement():
    from debvader_amd.measure import measurement as ms

    assert list(inspect.signature(ms.fit_fluxes).parameters) == ["stamps_mean", "places", "data_fields", "field_ptr", "catalogue",
                                                                 "sky_sigma", "min_pivot", "ctx"]
    assert inspect.signature(ms.fit_fluxes).parameters["min_pivot"].default == 1e-8
    P, places, D, truth = _pair()
    ctx = OracleContext()
    rec = ms.fit_fluxes(P, places, D, ctx=ctx)                    # one field given as (F, F, bands)
    assert ctx.calls[-1] == dict(fit_flux=2, fields=1, min_pivot=1e-8, field_ptr=[0, 2])
    flux = P.sum(axis=(1, 2), dtype=np.float64)
    assert np.abs(rec["fit_scale"] - truth[:, None]).max() < 1e-11 and np.array_equal(rec["flux_fit"], rec["fit_scale"] * flux)
    assert np.isnan(rec["flux_fit_err"]).all()
    # two fields, the catalogue's flux, the sky per field
    cat = np.recarray((4,), dtype=[("flux", "<f8", (3,))])
    cat["flux"] = np.arange(12.0).reshape(4, 3) - 3.0
    sky = np.array([[0.1, 0.2, 0.3], [0.4, 0.5, 0.6]])
    P4, pl4 = np.concatenate([P, P[::-1]]), np.concatenate([places, places[::-1]])
    rec = ms.fit_fluxes(P4, pl4, np.stack([D, D]), field_ptr=[0, 2, 4], catalogue=cat, sky_sigma=sky, min_pivot=1e-6, ctx=ctx)
    assert ctx.calls[-1] == dict(fit_flux=4, fields=2, min_pivot=1e-6, field_ptr=[0, 2, 4])
    assert np.array_equal(rec["flux_fit"], rec["fit_scale"] * cat["flux"])
    assert np.array_equal(rec["fit_scale_err"], sky[[0, 0, 1, 1]] * np.sqrt(rec["fit_var"]))
    assert np.abs(rec["fit_scale"][[3, 2]] - truth[:, None]).max() < 1e-11
    n_calls = len(ctx.calls)
    with pytest.raises(ValueError, match="lacks the column flux"):
        ms.fit_fluxes(P, places, D, catalogue=np.recarray((2,), dtype=[("row", "<f8")]), ctx=ctx)
    with pytest.raises(ValueError, match="sky_sigma must have shape"):
        ms.fit_fluxes(P, places, D, sky_sigma=[0.1, 0.2], ctx=ctx)
    with pytest.raises(ValueError, match="finite and positive"):
        ms.fit_fluxes(P, places, D, sky_sigma=[0.1, 0.0, 0.1], ctx=ctx)
    assert len(ctx.calls) == n_calls


F = 81
DIST = [np.array([[0.0, 0.0], [5.0, -7.0]]), np.zeros((0, 2)), np.array([[100.0, 0.0], [-3.0, 11.0]]), np.array([[0.0, 40.0]])]


def _batch():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch

    net = Net()
    return net, DeblendFieldBatch(net, np.random.default_rng(3).normal(size=(4, F, F, NB)), CS, NB)


def test_deblend_fields_appends_the_fit_flux_columns():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch
    from debvader_amd.measure import measurement as ms

    sig = inspect.signature(DeblendFieldBatch.deblend_fields).parameters
    assert sig["fit_flux"].default is False and sig["fit_flux"].kind is inspect.Parameter.KEYWORD_ONLY
    assert DeblendFieldBatch.fit_flux_columns(NB) == ms.fit_flux_dtype(NB)
    net, b = _batch()
    sky_fields = np.arange(1, 4 * NB + 1, dtype=np.float64).reshape(4, NB)
    want = np.dtype(DeblendFieldBatch.ON_DEVICE_COLUMNS + DeblendFieldBatch.measure_columns(NB) + DeblendFieldBatch.fit_flux_columns(NB))
    for sky in (None, np.full(NB, 0.3), sky_fields):
        for rf in (True, False):
            res = b.deblend_fields(DIST, on_device=True, measure=True, fit_flux=True, sky_sigma=sky, return_fields=rf)
            call = net._core.engine.calls[-2]
            assert call[0] == "infer_fields_measure_fit" and call[2] is rf and call[3] is not None       # places: always
            assert [len(r) for r in res] == [2, 0, 1, 0] and all(r.dtype == want for r in res)
            f, c = stub_fit_flux(3, NB), stub_catalogue(3, NB)
            cat = ms.fit_flux_records(*(f[k] for k in KEYS), c["flux"], sky_sigma=sky, field_ptr=[0, 2, 2, 3, 3])
            for i, (m, k) in enumerate([(0, 0), (0, 1), (2, 0)]):
                for n in cat.dtype.names:
                    assert np.array_equal(res[m][n][k], cat[n][i], equal_nan=True), n
                assert np.array_equal(res[m]["flux"][k], c["flux"][i])
            assert res[0]["fit_status"][1, 0] == 5 and res[0]["flux_fit"][1, 0] == c["flux"][1, 0]
            assert (sky is None) == bool(np.isnan(res[0]["flux_fit_err"][0]).all())
            if sky is sky_fields:
                assert np.array_equal(res[2]["fit_scale_err"][0], sky_fields[2] * np.sqrt(f["fit_var"][2]))
    # without fit_flux the call and the columns are those of before
    res = b.deblend_fields(DIST, on_device=True, measure=True)
    assert net._core.engine.calls[-2][0] == "infer_fields_measure" and "fit_scale" not in res[0].dtype.names


def test_deblend_fields_refuses_fit_flux_combinations():
    net, b = _batch()
    on = dict(on_device=True, measure=True)
    for kw, match in ((dict(fit_flux=True), "fit_flux=True needs measure=True and on_device=True"),
                      (dict(fit_flux=True, measure=True), "fit_flux=True needs measure=True and on_device=True"),
                      (dict(fit_flux=True, on_device=True), "fit_flux=True needs measure=True and on_device=True"),
                      (dict(fit_flux=True, psf=np.ones((21, 21)), **on), "fit_flux=True cannot be combined with psf"),
                      (dict(fit_flux=True, apertures=(3.0,), **on), "fit_flux=True cannot be combined with apertures"),
                      (dict(fit_flux=True, apertures=(3.0,), aperture_data=True, **on), "fit_flux=True cannot be combined with apertures"),
                      (dict(fit_flux=True, blendedness=True, **on), "fit_flux=True cannot be combined with blendedness"),
                      (dict(fit_flux=True, measure_samples=4, **on), "fit_flux=True cannot be combined with measure_samples"),
                      (dict(fit_flux=True, optimise_positions=True, **on), "fit_flux=True cannot be combined with optimise_positions"),
                      (dict(fit_flux=True, epistemic_uncertainty_estimation=True, **on),
                       "fit_flux=True cannot be combined with epistemic_uncertainty_estimation"),
                      (dict(fit_flux=True, sky_sigma=np.ones(NB + 1), **on), "sky_sigma must have shape"),
                      (dict(fit_flux=True, sky_sigma=np.ones((3, NB)), **on), "sky_sigma must have shape"),
                      (dict(fit_flux=True, sky_sigma=np.zeros(NB), **on), "finite and positive"),
                      # sky_sigma with neither aperture_data nor fit_flux keeps raising as it did
                      (dict(sky_sigma=np.ones(NB), **on), "give aperture_data too"),
                      (dict(sky_sigma=np.ones(NB), apertures=(3.0,), **on), "give aperture_data too")):
        with pytest.raises(ValueError, match=match):
            b.deblend_fields(DIST, **kw)
    assert not [c for c in net._core.engine.calls if c[0].startswith("infer")]


def test_engine_wrappers_refuse_before_the_library():
    from debvader_amd import engine as E

    P, pl, D = np.zeros((2, 31, 31, 3), np.float32), np.zeros((2, 2), np.int32), np.zeros((1, 40, 40, 3))
    call = lambda *a, **kw: E.Context.scene_fit_flux(object(), *a, **kw)     # noqa: E731
    for args, kw, match in (((P[0], pl, D), {}, "expected square stamps"),
                            ((np.zeros((2, 31, 30, 3)), pl, D), {}, "expected square stamps"),
                            ((P, pl, D[0]), {}, "expected data fields"),
                            ((P, pl, np.zeros((1, 40, 40, 2))), {}, "expected data fields"),
                            ((P, pl, np.zeros((1, 40, 41, 3))), {}, "expected data fields"),
                            ((P, pl[:1], D), {}, r"expected places \(2, 2\)"),
                            ((P, pl + 0.5, D), {}, "must be integers"),
                            ((P, pl, np.zeros((2, 40, 40, 3))), {}, "field_ptr is needed"),
                            ((P, pl, D), dict(field_ptr=[0, 1]), "field_ptr must start at 0 and end"),
                            ((P, pl, np.zeros((2, 40, 40, 3))), dict(field_ptr=[0, 3, 2]), "must not decrease"),
                            ((P, pl, D), dict(min_pivot=0.0), "min_pivot"), ((P, pl, D), dict(min_pivot=1.0), "min_pivot"),
                            ((P, pl, D), dict(min_pivot=float("nan")), "min_pivot"),
                            ((P, pl, D), dict(scratch_bytes=0), "scratch_bytes"),
                            ((P, pl, D), dict(scratch_bytes=10.5), "scratch_bytes")):
        with pytest.raises(ValueError, match=match):
            call(*args, **kw)
    for kw, match in ((dict(places=None), "places are needed"), (dict(places=None, return_fields=False), "places are needed"),
                      (dict(places=[[0, 0]], min_pivot=2.0), "min_pivot"), (dict(places=[[0, 0]], scratch_bytes=-1), "scratch_bytes"),
                      (dict(places=[[0, 0]], band=7), "band")):
        places = kw.pop("places")
        with pytest.raises(ValueError, match=match):
            E.Engine.infer_fields_measure_fit(object(), np.zeros((1, 81, 81, 6)), [[0, 0]], [0, 1], places, **kw)
    with pytest.raises(ValueError, match="at most 1024"):
        E.Context.scene_fit_flux_gram(object(), np.zeros((1025, 3, 3, 1), np.float32), np.zeros((1025, 2), np.int32), np.zeros((8, 8, 1)))
    with pytest.raises(ValueError, match="expected one data field"):
        E.Context.scene_fit_flux_gram(object(), P, pl, D)
    par = E.fit_flux_params()
    assert par.min_pivot == 1e-8 and par.scratch_bytes == 256 << 20
    out, ptrs = E._fit_flux_out(4, 6)
    assert list(out) == list(E.FIT_FLUX_KEYS) == list(KEYS) and not any(p is None for p in ptrs)
    assert all(out[k].shape == (4, 6) for k in KEYS) and out["fit_status"].dtype == np.int32 and out["fit_var"].dtype == np.float64
    # an empty call returns without the library
    empty = call(P[:0], pl[:0], D)
    assert empty["fit_scale"].shape == (0, 3) and empty["fit_status"].dtype == np.int32
    assert E.Context.scene_fit_flux_gram(object(), P[:0], pl[:0], D[0])["gram"].shape == (3, 0, 0)


def _c_types(arglist):
    out = []
    for a in arglist.split(","):
        a = re.sub(r"/\*.*?\*/", "", a).replace("const", "").strip()
        out.append(re.sub(r"\s*\w+$", "", a).replace(" ", ""))
    return out


def test_header_binding_and_library_agree_on_the_new_entry_points():
    from debvader_amd import _lib

    header = open(os.path.join(ROOT, "include", "debvader_hip.h")).read()
    ctype = {"dv_model*": C.c_void_p, "dv_ctx*": C.c_void_p, "double*": C.POINTER(C.c_double), "float*": C.POINTER(C.c_float),
             "int32_t*": C.POINTER(C.c_int32), "int64_t*": C.POINTER(C.c_int64), "int32_t": C.c_int32, "int64_t": C.c_int64,
             "uint64_t": C.c_uint64, "double": C.c_double, "dv_measure_params*": C.POINTER(_lib.DvMeasureParams),
             "dv_fit_flux_params*": C.POINTER(_lib.DvFitFluxParams)}
    for name, nargs in (("dv_fit_flux_params_default", 1), ("dv_scene_fit_flux", 16), ("dv_scene_fit_flux_gram", 10),
                        ("dv_infer_fields_measure_fit", 26)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header, re.S)
        assert m, f"{name} is not declared in include/debvader_hip.h"
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)         # bound: the library exports it
        restype, argtypes = _lib.SIGNATURES[name]
        want = [ctype[t] for t in _c_types(m.group(1))]
        assert restype is C.c_int and len(argtypes) == len(want) == nargs
        for i, (a, w) in enumerate(zip(argtypes, want)):
            assert a is w, (name, i, a, w)
        assert getattr(_lib.lib, name).argtypes == argtypes
    # dv_infer_fields_measure's arguments, then the params and the five outputs of dv_scene_fit_flux
    assert _lib.SIGNATURES["dv_infer_fields_measure_fit"][1][:20] == _lib.SIGNATURES["dv_infer_fields_measure"][1]
    assert _lib.SIGNATURES["dv_infer_fields_measure_fit"][1][20:] == _lib.SIGNATURES["dv_scene_fit_flux"][1][10:]
    # the struct is the header's, the default the documented one (no GPU is touched)
    m = re.search(r"typedef struct dv_fit_flux_params \{(.*?)\} dv_fit_flux_params;", header, re.S)
    fields = re.findall(r"(double|int64_t)\s+(\w+);", m.group(1))
    assert [(n, {"double": C.c_double, "int64_t": C.c_int64}[t]) for t, n in fields] == list(_lib.DvFitFluxParams._fields_)
    par = _lib.DvFitFluxParams()
    assert _lib.lib.dv_fit_flux_params_default(C.byref(par)) == 0 and par.min_pivot == 1e-8 and par.scratch_bytes == 256 << 20
    assert re.search(r"#define DV_FIT_MAX_N 1024\b", header)
    # every existing entry point keeps its signature
    for name, nargs in (("dv_infer_fields_measure", 20), ("dv_infer_fields_measure_blend", 22), ("dv_infer_fields_measure_aper", 30),
                        ("dv_infer_fields_measure_aper_data", 36), ("dv_scene_blend", 16)):
        assert len(_lib.SIGNATURES[name][1]) == nargs
    kernel = open(os.path.join(ROOT, "debvader_amd", "csrc", "fitflux.hip")).read()
    assert "fitflux_gram_kernel" in kernel and "fitflux_solve_kernel" in kernel and "#pragma clang fp contract(off)" in kernel
    assert "getenv" not in kernel and "atomic" not in kernel.replace("No atomics", "")
    assert "fitflux.hip" in open(os.path.join(ROOT, "debvader_amd", "csrc", "Makefile")).read()
    engine = open(os.path.join(ROOT, "debvader_amd", "csrc", "engine.hip")).read()
    assert "launch_fit_flux(" in engine and "struct FitFluxStage" in engine
