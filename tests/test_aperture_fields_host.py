"""CPU checks of the apertures on the fields: the numpy restatement of the definition
(tests/aperture_fields_oracle.py) on inputs whose answer is known, the Python layer -
debvader_amd.measure.measurement.measure_apertures_on_fields / aperture_data_records and
DeblendFieldBatch.deblend_fields(measure=True, apertures=..., aperture_data=True) - over the stand-in engine of
tests/stub_aperture_fields_engine.py, and the ABI.  No GPU is touched."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import numpy.lib.recfunctions as rfn
import pytest

from tests import aperture_fields_oracle as afo
from tests import aperture_oracle as ao
from tests import measure_oracle as mo
from tests.stub_aperture_engine import stub_aperture
from tests.stub_aperture_fields_engine import CS, NB, Net, OracleContext, stub_aperture_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS31, F64, NB3 = 31, 64, 3
PAR = ao.params()                                  # radii 3, 5, 8; 5 x 5 sub-pixels
BANDS = np.array([0.6, 1.3, 1.0])


def _stamp(M, off, amp=1.0, cs=CS31):
    """a noise-free elliptical Gaussian in three bands, as the float32 the network would give"""
    return (amp * mo.gaussian_stamp(cs, M, off)[:, :, None] * BANDS).astype(np.float32)


def _rows(P, par=PAR):
    """(catalogue shape, status, aperture row) of one stamp, measured by the restatements"""
    sh, _, st = mo.adaptive_moments(P[:, :, 2].astype(np.float64))
    return sh, st, ao.aperture_row(P, None, sh, st, 2, par, True)


def _records(rows, aps, band=2, **kw):
    from debvader_amd.measure import measurement as ms

    return ms.aperture_data_records(*(afo.stack(rows, k) for k in afo.KEYS), np.stack([a["ap_flux"] for a in aps]),
                                    np.stack([a["ap_area"] for a in aps]), np.stack([a["flux_auto"] for a in aps]),
                                    np.array([a["kron"][2] for a in aps]), band=band, **kw)


def _pair(model_amp):
    """two galaxies 6 px apart in one 64-px field: (G stamps, P stamps, places, D, T)"""
    G = [_stamp((4.0, 0.8, 3.0), (0.21, -0.33)), _stamp((5.0, -1.0, 3.5), (-0.4, 0.17), amp=1.7)]
    P = [(np.float32(model_amp) * G[0]).astype(np.float32), G[1]]
    places = np.array([[16, 14], [16, 20]])
    return G, P, places, afo.composite(G, places, F64), afo.composite(P, places, F64)


def test_a_biased_model_does_not_bias_the_data_flux():
    """D = G1 + G2, P1 = 0.9 G1, P2 = G2: the model flux of galaxy 1 is 10 % low, sum w (D - T + P1) is sum w G1 to the
    rounding of the three sums"""
    G, P, places, D, T = _pair(0.9)
    sh, st, ap = _rows(P[0])
    assert st == 0 and ap["status"] == ao.OK and ap["flags"] & 0x1ff == 0
    row = afo.field_row(sh, st, ap["status"], ap["kron"][1], places[0], T, D, CS31, PAR, True)
    truth = afo.field_row(sh, st, ap["status"], ap["kron"][1], places[0], afo.composite(G[:1], places[:1], F64), None, CS31, PAR, True)
    rec = _records([row], [ap])
    assert np.array_equal(rec["ap_field_area"][0], ap["ap_area"]) and rec["auto_field_area"][0] == ap["kron"][2]
    assert rec["aper_data_flags"][0] == 0
    worst = 0.0
    for got, want, scale in ((rec["ap_flux_data"][0], truth["ap_model_sum"], ap["ap_abs"] + row["ap_model_abs"] + row["ap_data_abs"]),
                             (rec["flux_auto_data"][0], truth["auto_model_sum"],
                              ap["auto_abs"] + row["auto_model_abs"] + row["auto_data_abs"])):
        worst = max(worst, float(np.max(np.abs(got - want) / scale)))
    print("data flux against sum w G1, relative to the absolute sums:", worst)
    assert worst <= 1e-12
    # the model flux stays 10 % low (0.9 rounded to float32 and the product rounded to float32: 1e-7)
    assert np.all(np.abs(ap["ap_flux"] / truth["ap_model_sum"] - 0.9) < 1e-6)
    assert np.all(np.abs(ap["flux_auto"] / truth["auto_model_sum"] - 0.9) < 1e-6)
    assert np.all(np.abs(rec["ap_flux_data"][0] / truth["ap_model_sum"] - 1.0) < 1e-12)
    # without the observed field the data columns are NaN, the model sums keep their bits
    nodata = afo.field_row(sh, st, ap["status"], ap["kron"][1], places[0], T, None, CS31, PAR, True)
    assert np.all(np.isnan(nodata["ap_data_sum"])) and np.all(np.isnan(nodata["auto_data_sum"]))
    assert np.array_equal(nodata["ap_model_sum"], row["ap_model_sum"])
    assert np.all(np.isnan(_records([nodata], [ap])["ap_flux_data"]))


def test_identities_of_an_unbiased_model_and_of_a_lone_galaxy():
    G, P, places, D, T = _pair(1.0)
    assert np.array_equal(D, T)
    for i in (0, 1):
        sh, st, ap = _rows(P[i])
        row = afo.field_row(sh, st, ap["status"], ap["kron"][1], places[i], T, D, CS31, PAR, True)
        assert np.array_equal(row["ap_data_sum"], row["ap_model_sum"]) and np.array_equal(row["auto_data_sum"], row["auto_model_sum"])
        rec = _records([row], [ap])
        assert np.array_equal(rec["ap_flux_data"][0], ap["ap_flux"]) and np.array_equal(rec["flux_auto_data"][0], ap["flux_auto"])
        assert np.all(rec["ap_blendedness"][0] > 0.0) and np.all(rec["ap_blendedness"][0] < 1.0)
    # alone in its field, the stamp inside it: T holds the widened stamp values, the raster sums are the same sums
    for place in ((16, 14), (0, 0), (F64 - CS31, F64 - CS31)):
        sh, st, ap = _rows(P[1])
        alone = afo.composite(P[1:], [place], F64)
        row = afo.field_row(sh, st, ap["status"], ap["kron"][1], place, alone, alone, CS31, PAR, True)
        assert np.array_equal(row["ap_model_sum"], ap["ap_flux"]) and np.array_equal(row["auto_model_sum"], ap["flux_auto"])
        assert np.array_equal(row["ap_field_area"], ap["ap_area"]) and row["auto_field_area"] == ap["kron"][2]
        rec = _records([row], [ap])
        assert np.all(rec["ap_blendedness"][0] == 0.0) and rec["auto_blendedness"][0] == 0.0
        assert rec["aper_data_flags"][0] == 0


def test_blendedness_in_the_apertures_falls_with_separation():
    """two equal round Gaussians: half of the model inside any aperture is the neighbour's at zero separation, less and less
    of it as they part"""
    P = _stamp((4.0, 0.0, 4.0), (0.0, 0.0))
    sh, st, ap = _rows(P)
    series = []
    for sep in (0, 1, 2, 4, 6, 9, 13):
        places = np.array([[16, 14], [16, 14 + sep]])
        T = afo.composite([P, P], places, F64)
        row = afo.field_row(sh, st, ap["status"], ap["kron"][1], places[0], T, None, CS31, PAR, True)
        rec = _records([row], [ap])
        series.append(np.concatenate([rec["ap_blendedness"][0], [rec["auto_blendedness"][0]]]))
    series = np.array(series)
    print("blendedness by separation (R = 3, 5, 8, auto):", series.tolist())
    assert np.all(np.abs(series[0] - 0.5) < 1e-12)
    assert np.all(np.diff(series, axis=0) < 0.0) and np.all(series[-1] < 0.02) and np.all(series > 0.0)
    # the small aperture sees less of the neighbour than the large one once they have parted
    assert series[4, 0] < series[4, 1] < series[4, 2]


def test_field_edges_truncate_and_flag():
    P = _stamp((4.0, 0.5, 3.0), (0.3, 0.2))
    sh, st, ap = _rows(P)
    # over the corner: the galaxy's centre (15.3, 15.2) lands on field pixel (2.3, 4.2) - every circle and the ellipse are cut
    place = (-13, -11)
    T = afo.composite([P], [place], F64)
    row = afo.field_row(sh, st, ap["status"], ap["kron"][1], place, T, T, CS31, PAR, True)
    assert np.all(row["ap_field_area"] < ap["ap_area"]) and row["auto_field_area"] < ap["kron"][2]
    assert np.all(row["ap_field_area"] > 0.0) and np.all(row["ap_model_sum"] < ap["ap_flux"])
    rec = _records([row], [ap])
    assert rec["aper_data_flags"][0] == 0b111 | 1 << 8
    assert np.all(rec["ap_blendedness"][0] < 0.0)          # the model part reaches further than the field: what the flag says
    # at an edge, far enough for the 3-px circle: bit 0 stays clear
    place = (-12, 20)                                      # centre on field row 3.3
    T = afo.composite([P], [place], F64)
    row = afo.field_row(sh, st, ap["status"], ap["kron"][1], place, T, T, CS31, PAR, True)
    assert row["ap_field_area"][0] == ap["ap_area"][0] and np.array_equal(row["ap_model_sum"][0], ap["ap_flux"][0])
    assert _records([row], [ap])["aper_data_flags"][0] == 0b110 | 1 << 8
    # wholly outside: nothing is summed
    for place in ((-CS31, 10), (10, F64), (-40, -40), (F64 + 5, F64 + 5)):
        T = np.ones((F64, F64, NB3))
        row = afo.field_row(sh, st, ap["status"], ap["kron"][1], place, T, T, CS31, PAR, True)
        for k in afo.KEYS:
            assert np.all(np.asarray(row[k]) == 0.0), (place, k)
        assert np.all(np.isnan(_records([row], [ap])["ap_blendedness"]))        # the denominator is not positive


def test_status_4_and_7_rows():
    P = _stamp((4.0, 0.0, 4.0), (0.2, 0.1))
    sh, st, ap = _rows(P)
    T = afo.composite([P], [(16, 14)], F64)
    for args in ((sh, 3, ao.INELIGIBLE), (sh, 0, ao.INELIGIBLE), ((np.nan,) + tuple(sh[1:]), 0, ao.OK),
                 ((15.0, 15.0, 1e-3, 0.0, 1e-4), 0, ao.OK)):
        row = afo.field_row(args[0], args[1], args[2], ap["kron"][1], (16, 14), T, T, CS31, PAR, True)
        for k in afo.KEYS:
            assert np.all(np.isnan(row[k])), k
    row = afo.field_row(sh, st, ao.NO_KRON, np.nan, (16, 14), T, T, CS31, PAR, True)
    for k in afo.KEYS:
        assert np.all(np.isnan(row[k])) == k.startswith("auto_"), k
    assert np.array_equal(row["ap_model_sum"], ap["ap_flux"])
    assert afo.field_row(sh, 2, ao.OK, ap["kron"][1], (16, 14), T, T, CS31, PAR, True)["auto_field_area"] == ap["kron"][2]
    # the derived columns follow: a row without Kron radius keeps its circles
    nokron = dict(ap, flux_auto=np.full(NB3, np.nan), kron=np.full(3, np.nan))
    rec = _records([row], [nokron])
    assert np.all(rec["ap_blendedness"][0] == 0.0) and np.isnan(rec["auto_blendedness"][0]) and np.all(np.isnan(rec["flux_auto_data"][0]))
    assert rec["aper_data_flags"][0] == 0


def test_one_sub_pixel_and_no_radii():
    rng = np.random.default_rng(8)
    T = rng.uniform(0.5, 1.5, size=(40, 40, NB3))
    D = rng.uniform(0.5, 1.5, size=(40, 40, NB3))
    sh = (10.3, 9.6, 4.0, 0.5, 3.0)
    par = ao.params(radii=(4.0,), subsample=1)
    row = afo.field_row(sh, 0, ao.OK, 2.0, (-8, 25), T, D, 21, par)
    r, c = np.mgrid[0:21, 0:21]
    infield = (r - 8 >= 0) & (c + 25 < 40)
    inside = ((r - 10.3) ** 2 + (c - 9.6) ** 2 <= 16.0) & infield
    assert row["ap_field_area"][0] == inside.sum() and inside.sum() < ((r - 10.3) ** 2 + (c - 9.6) ** 2 <= 16.0).sum()
    assert np.allclose(row["ap_model_sum"][0], T[r[inside] - 8, c[inside] + 25].sum(axis=0), rtol=1e-13, atol=0)
    assert np.allclose(row["ap_data_sum"][0], D[r[inside] - 8, c[inside] + 25].sum(axis=0), rtol=1e-13, atol=0)
    det = 4.0 * 3.0 - 0.25
    q = (3.0 / det) * (r - 10.3) ** 2 + (-1.0 / det) * (r - 10.3) * (c - 9.6) + (4.0 / det) * (c - 9.6) ** 2
    assert row["auto_field_area"] == ((q <= 4.0) & infield).sum()
    none = afo.field_row(sh, 0, ao.OK, 2.0, (-8, 25), T, D, 21, ao.params(radii=(), subsample=1))
    assert none["ap_model_sum"].shape == (0, NB3) and none["ap_field_area"].shape == (0,)
    assert np.array_equal(none["auto_model_sum"], row["auto_model_sum"]) and none["auto_field_area"] == row["auto_field_area"]
    # the shortcut of the count changes nothing
    full = afo.field_row(sh, 0, ao.OK, 2.0, (-8, 25), T, D, 21, ao.params(radii=(4.0, 7.5)), False)
    short = afo.field_row(sh, 0, ao.OK, 2.0, (-8, 25), T, D, 21, ao.params(radii=(4.0, 7.5)), True)
    for k in afo.KEYS:
        assert np.array_equal(full[k], short[k]), k


# ---- the host layer over the stand-in engine ----------------------------------------------------------------------------------

GPU_COLUMNS = list(afo.KEYS)
DERIVED = ["ap_flux_data", "flux_auto_data", "ap_blendedness", "auto_blendedness", "aper_data_flags", "ap_flux_data_err",
           "flux_auto_data_err"]


def test_aperture_data_records_columns_and_derived_values():
    from debvader_amd.measure import measurement as ms

    assert [c[0] for c in ms.aperture_data_dtype(6, 3)] == GPU_COLUMNS + DERIVED
    dt = np.dtype(ms.aperture_data_dtype(6, 2))
    assert dt["ap_model_sum"].shape == (2, 6) and dt["ap_field_area"].shape == (2,) and dt["auto_data_sum"].shape == (6,)
    assert dt["ap_flux_data"].shape == (2, 6) and dt["ap_blendedness"].shape == (2,) and dt["aper_data_flags"] == np.int32
    assert dt["ap_flux_data_err"].shape == (2, 6) and dt["flux_auto_data_err"].shape == (6,) and dt["auto_field_area"].shape == ()
    n, nb, K = 6, 6, 3
    a, f = stub_aperture(n, nb, K, 0), stub_aperture_fields(n, nb, K)
    args = [f[k] for k in afo.KEYS] + [a["ap_flux"], a["ap_area"], a["flux_auto"], a["kron"][:, 2]]
    rec = ms.aperture_data_records(*args)
    for k in afo.KEYS:
        assert np.array_equal(rec[k], f[k], equal_nan=True), k
    assert a["aper_status"].tolist() == [0, 7, 0, 0, 4, 0]
    ok = [0, 2, 3, 5]
    assert np.array_equal(rec["ap_flux_data"][ok], a["ap_flux"][ok] + (f["ap_data_sum"][ok] - f["ap_model_sum"][ok]))
    assert np.array_equal(rec["ap_flux_data"][ok], a["ap_flux"][ok] + 2.0)
    assert np.array_equal(rec["flux_auto_data"][ok], a["flux_auto"][ok] - 0.5)
    # 1 - ap_flux / (1.25 ap_flux) = 0.2 where ap_flux[band] is positive; row 0, circle 0 has ap_flux[2] = 2
    assert np.allclose(rec["ap_blendedness"][ok], 0.2, rtol=1e-15) and np.allclose(rec["auto_blendedness"][ok], 0.5, rtol=1e-15)
    assert rec["aper_data_flags"].tolist() == [0, 0, 1, 1 << 8, 0, 0]
    assert np.all(np.isnan(rec["ap_flux_data_err"])) and np.all(np.isnan(rec["flux_auto_data_err"]))
    # NaN follows the GPU's: row 1 (no Kron radius) keeps its circles, row 4 (ineligible) has nothing
    assert np.all(np.isnan(rec["flux_auto_data"][1])) and np.isnan(rec["auto_blendedness"][1]) and not np.isnan(rec["ap_flux_data"][1]).any()
    for k in DERIVED:
        if k != "aper_data_flags":
            assert np.all(np.isnan(rec[k][4])), k
    # a denominator that is not positive gives NaN, in the chosen band only
    f0 = {k: v.copy() for k, v in f.items()}
    f0["ap_model_sum"][0, 1, 2] = 0.0
    f0["ap_model_sum"][2, 0, 2] = -3.0
    f0["auto_model_sum"][3, 0] = 0.0
    r0 = ms.aperture_data_records(*([f0[k] for k in afo.KEYS] + args[6:]))
    assert np.isnan(r0["ap_blendedness"][0, 1]) and np.isnan(r0["ap_blendedness"][2, 0]) and not np.isnan(r0["ap_blendedness"][0, 0])
    assert not np.isnan(r0["auto_blendedness"][3])
    assert np.isnan(ms.aperture_data_records(*([f0[k] for k in afo.KEYS] + args[6:]), band=0)["auto_blendedness"][3])
    with pytest.raises(ValueError, match="band 6"):
        ms.aperture_data_records(*args, band=6)
    # no radii
    a0, g0 = stub_aperture(n, nb, 0, 0), stub_aperture_fields(n, nb, 0)
    rz = ms.aperture_data_records(*([g0[k] for k in afo.KEYS] + [a0["ap_flux"], a0["ap_area"], a0["flux_auto"], a0["kron"][:, 2]]))
    assert rz["ap_flux_data"].shape == (n, 0, nb) and rz["ap_blendedness"].shape == (n, 0)
    assert np.array_equal(rz["flux_auto_data"], rec["flux_auto_data"], equal_nan=True)
    assert rz["aper_data_flags"].tolist() == [0, 0, 0, 1 << 8, 0, 0]


def test_sky_sigma_gives_the_errors():
    from debvader_amd.measure import measurement as ms

    n, nb, K = 6, 6, 3
    a, f = stub_aperture(n, nb, K, 0), stub_aperture_fields(n, nb, K)
    args = [f[k] for k in afo.KEYS] + [a["ap_flux"], a["ap_area"], a["flux_auto"], a["kron"][:, 2]]
    sky = np.linspace(0.1, 0.6, nb)
    rec = ms.aperture_data_records(*args, sky_sigma=sky)
    assert np.array_equal(rec["ap_flux_data_err"], sky[None, None, :] * np.sqrt(f["ap_field_area"])[:, :, None], equal_nan=True)
    assert np.array_equal(rec["flux_auto_data_err"], sky[None, :] * np.sqrt(f["auto_field_area"])[:, None], equal_nan=True)
    assert np.all(np.isnan(rec["flux_auto_data_err"][[1, 4]])) and not np.isnan(rec["ap_flux_data_err"][1]).any()
    fp = [0, 2, 2, 5, 6]
    sky2 = np.arange(1, 4 * nb + 1, dtype=np.float64).reshape(4, nb)
    rec2 = ms.aperture_data_records(*args, sky_sigma=sky2, field_ptr=fp)
    fld = [0, 0, 2, 2, 2, 3]
    assert np.array_equal(rec2["flux_auto_data_err"], sky2[fld] * np.sqrt(f["auto_field_area"])[:, None], equal_nan=True)
    assert np.array_equal(rec2["ap_flux_data_err"], sky2[fld][:, None, :] * np.sqrt(f["ap_field_area"])[:, :, None], equal_nan=True)
    same = ms.aperture_data_records(*args, sky_sigma=sky, field_ptr=fp)
    assert np.array_equal(same["ap_flux_data_err"], rec["ap_flux_data_err"], equal_nan=True)
    for bad, match in ((np.ones(nb + 1), "must have shape"), (np.ones((3, nb)), "must have shape"), (np.ones((4, nb, 1)), "must have shape"),
                       (np.zeros(nb), "finite and positive"), (-sky, "finite and positive"),
                       (np.where(np.arange(nb) == 1, np.nan, sky), "finite and positive"),
                       (np.where(np.arange(nb) == 1, np.inf, sky), "finite and positive")):
        with pytest.raises(ValueError, match=match):
            ms.aperture_data_records(*args, sky_sigma=bad, field_ptr=fp)
    with pytest.raises(ValueError, match="field_ptr must start at 0"):
        ms.aperture_data_records(*args, sky_sigma=sky, field_ptr=[0, 3, 2, 6])
    assert ms.check_sky_sigma(sky, 4, nb).shape == (4, nb)


def test_measure_apertures_on_fields_over_the_restatements():
    from debvader_amd.measure import measurement as ms

    sig = inspect.signature(ms.measure_apertures_on_fields).parameters
    assert list(sig)[:6] == ["catalogue", "places", "model_fields", "data_fields", "field_ptr", "sky_sigma"]
    assert sig["data_fields"].default is None and sig["field_ptr"].default is None and sig["sky_sigma"].default is None
    G, P, places, D, T = _pair(0.9)
    ctx = OracleContext()
    stamps = np.stack(P)
    cat = ms.measure_stamps(stamps, ctx=ctx)
    aps = ms.measure_apertures(stamps, catalogue=cat, ctx=ctx)
    ctx.calls.clear()
    rec = ms.measure_apertures_on_fields(cat, places, T, D, apertures=aps, cutout_size=CS31, ctx=ctx)
    assert len(ctx.calls) == 1 and ctx.calls[0]["aperture_fields"] == 2 and ctx.calls[0]["with_data"]
    assert ctx.calls[0]["radii"] == (3.0, 5.0, 8.0) and ctx.calls[0]["cutout_size"] == CS31 and ctx.calls[0]["field_ptr"] == [0, 2]
    assert rec.dtype == np.dtype(ms.aperture_data_dtype(NB3, 3)) and len(rec) == 2
    truth = ao.aperture_row(G[0], None, [cat[k][0] for k in ("row", "col", "Mrr", "Mrc", "Mcc")], 0, 2, PAR, True)
    assert np.allclose(rec["ap_flux_data"][0], truth["ap_flux"], rtol=1e-11, atol=0)
    assert np.allclose(aps["ap_flux"][0], 0.9 * truth["ap_flux"], rtol=1e-6, atol=0)
    assert np.all(rec["ap_blendedness"] > 0) and np.all(np.isnan(rec["ap_flux_data_err"]))
    # one catalogue with both sets of columns (as deblend_fields gives), several fields, a sky level, no observed field
    both = rfn.merge_arrays([np.asarray(cat), np.asarray(aps)], flatten=True, asrecarray=True)
    rec2 = ms.measure_apertures_on_fields(both, places, np.stack([T, T]), field_ptr=[0, 1, 2], sky_sigma=[[0.1] * 3, [0.2] * 3],
                                          cutout_size=CS31, ctx=ctx)
    assert ctx.calls[-1]["field_ptr"] == [0, 1, 2] and not ctx.calls[-1]["with_data"]
    assert np.array_equal(rec2["ap_model_sum"], rec["ap_model_sum"]) and np.all(np.isnan(rec2["ap_flux_data"]))
    assert np.array_equal(rec2["flux_auto_data_err"][1], 0.2 * np.sqrt(rec2["auto_field_area"][1]) * np.ones(3))
    # refusals
    n_calls = len(ctx.calls)
    with pytest.raises(ValueError, match="lacks the columns"):
        ms.measure_apertures_on_fields(cat, places, T, D, cutout_size=CS31, ctx=ctx)
    with pytest.raises(ValueError, match="2 radii given"):
        ms.measure_apertures_on_fields(both, places, T, D, radii=(3.0, 5.0), cutout_size=CS31, ctx=ctx)
    with pytest.raises(ValueError, match="sky_sigma must have shape"):
        ms.measure_apertures_on_fields(both, places, T, D, sky_sigma=[0.1, 0.2], cutout_size=CS31, ctx=ctx)
    with pytest.raises(ValueError, match="finite and positive"):
        ms.measure_apertures_on_fields(both, places, T, D, sky_sigma=[0.1, 0.0, 0.1], cutout_size=CS31, ctx=ctx)
    assert len(ctx.calls) == n_calls


F = 81
DIST = [np.array([[0.0, 0.0], [5.0, -7.0]]), np.zeros((0, 2)), np.array([[100.0, 0.0], [-3.0, 11.0]]), np.array([[0.0, 40.0]])]


def _batch():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch

    net = Net()
    return net, DeblendFieldBatch(net, np.random.default_rng(3).normal(size=(4, F, F, NB)), CS, NB)


def test_deblend_fields_appends_the_aperture_data_columns():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch
    from debvader_amd.measure import measurement as ms

    sig = inspect.signature(DeblendFieldBatch.deblend_fields).parameters
    assert sig["aperture_data"].default is False and sig["sky_sigma"].default is None
    assert DeblendFieldBatch.aperture_data_columns(NB, 2) == ms.aperture_data_dtype(NB, 2)
    net, b = _batch()
    sky_fields = np.arange(1, 4 * NB + 1, dtype=np.float64).reshape(4, NB)
    for apertures, K, sky in (((3.0, 5.0, 8.0), 3, None), ((), 0, np.full(NB, 0.3)), ((4.0,), 1, sky_fields)):
        want = np.dtype(DeblendFieldBatch.ON_DEVICE_COLUMNS + DeblendFieldBatch.measure_columns(NB) +
                        DeblendFieldBatch.aperture_columns(NB, K, 3) + DeblendFieldBatch.aperture_data_columns(NB, K))
        for rf in (True, False):
            res = b.deblend_fields(DIST, on_device=True, measure=True, apertures=apertures, aperture_data=True, sky_sigma=sky,
                                   return_fields=rf)
            call = net._core.engine.calls[-2]
            assert call[0] == "infer_fields_measure_aper_data" and call[2] is rf and call[3] is not None     # places: always
            assert call[4] == tuple(float(r) for r in apertures) and call[5] == (0.2, 0.5, 0.8)
            assert [len(r) for r in res] == [2, 0, 1, 0] and all(r.dtype == want for r in res)
            a, f = stub_aperture(3, NB, K, 3), stub_aperture_fields(3, NB, K)
            cat = ms.aperture_data_records(*[f[k] for k in afo.KEYS], a["ap_flux"], a["ap_area"], a["flux_auto"], a["kron"][:, 2],
                                           sky_sigma=sky, field_ptr=[0, 2, 2, 3, 3])
            for i, (m, k) in enumerate([(0, 0), (0, 1), (2, 0)]):
                for n in cat.dtype.names:
                    assert np.array_equal(res[m][n][k], cat[n][i], equal_nan=True), n
            assert res[0]["aper_status"].tolist() == [0, 7] and np.all(np.isnan(res[0]["flux_auto_data"][1]))
            assert (sky is None) == bool(np.isnan(res[0]["flux_auto_data_err"][0]).all())
            if sky is sky_fields:
                assert np.array_equal(res[2]["flux_auto_data_err"][0], sky_fields[2] * np.sqrt(f["auto_field_area"][2]))
    # without aperture_data the call and the columns are those of before
    res = b.deblend_fields(DIST, on_device=True, measure=True, apertures=(3.0,))
    assert net._core.engine.calls[-2][0] == "infer_fields_measure_aper" and "ap_model_sum" not in res[0].dtype.names


def test_deblend_fields_refuses_aperture_data_combinations():
    net, b = _batch()
    on = dict(on_device=True, measure=True)
    for kw, match in ((dict(aperture_data=True, **on), "aperture_data=True needs apertures"),
                      (dict(aperture_data=True), "aperture_data=True needs apertures"),
                      (dict(sky_sigma=np.ones(NB), apertures=(3.0,), **on), "give aperture_data too"),
                      (dict(sky_sigma=np.ones(NB), **on), "give aperture_data too"),
                      (dict(sky_sigma=np.ones(NB + 1), apertures=(3.0,), aperture_data=True, **on), "sky_sigma must have shape"),
                      (dict(sky_sigma=np.ones((3, NB)), apertures=(3.0,), aperture_data=True, **on), "sky_sigma must have shape"),
                      (dict(sky_sigma=np.zeros(NB), apertures=(3.0,), aperture_data=True, **on), "finite and positive"),
                      (dict(sky_sigma=-np.ones((4, NB)), apertures=(3.0,), aperture_data=True, **on), "finite and positive"),
                      (dict(sky_sigma=np.full(NB, np.nan), apertures=(3.0,), aperture_data=True, **on), "finite and positive"),
                      # the refusals of apertures stay as they are
                      (dict(apertures=(3.0,), aperture_data=True), "need measure=True and on_device=True"),
                      (dict(apertures=(3.0,), aperture_data=True, psf=np.ones((21, 21)), **on), "cannot be combined with psf"),
                      (dict(apertures=(3.0,), aperture_data=True, blendedness=True, **on), "cannot be combined with blendedness"),
                      (dict(apertures=(3.0,), aperture_data=True, measure_samples=4, **on), "cannot be combined with measure_samples"),
                      (dict(apertures=(3.0,), aperture_data=True, on_device=True, measure=True, optimise_positions=True),
                       "cannot be combined with optimise_positions"),
                      (dict(apertures=(3.0,), aperture_data=True, on_device=True, measure=True, epistemic_uncertainty_estimation=True),
                       "cannot be combined with epistemic_uncertainty_estimation")):
        with pytest.raises(ValueError, match=match):
            b.deblend_fields(DIST, **kw)
    assert not [c for c in net._core.engine.calls if c[0].startswith("infer")]


def test_engine_wrappers_refuse_before_the_library():
    from debvader_amd import engine as E

    sh, s0, kr, pl = np.zeros((2, 5)), np.zeros(2, np.int32), np.zeros((2, 3)), np.zeros((2, 2), np.int32)
    T = np.zeros((1, 40, 40, 3))
    call = lambda *a, **kw: E.Context.scene_aperture_fields(object(), *a, **dict(dict(cutout_size=31), **kw))     # noqa: E731
    for args, kw, match in (((sh, s0, pl, kr, s0, T[0]), {}, "expected model fields"),
                            ((sh, s0, pl, kr, s0, np.zeros((1, 40, 41, 3))), {}, "expected model fields"),
                            ((sh, s0, pl, kr, s0, T, np.zeros((1, 40, 40, 2))), {}, "expected data fields"),
                            ((sh[:1], s0, pl, kr, s0, T), {}, r"expected shape \(N, 5\)"),
                            ((sh, s0, pl[:1], kr, s0, T), {}, r"expected shape \(N, 5\)"),
                            ((sh, s0, pl, kr[:, :2], s0, T), {}, r"expected shape \(N, 5\)"),
                            ((sh, s0, pl, kr, s0[:1], T), {}, r"expected shape \(N, 5\)"),
                            ((sh, s0, pl + 0.5, kr, s0, T), {}, "must be integers"),
                            ((sh, s0, pl, kr, s0, np.zeros((2, 40, 40, 3))), {}, "field_ptr is needed"),
                            ((sh, s0, pl, kr, s0, T), dict(field_ptr=[0, 1]), "field_ptr must start at 0 and end"),
                            ((sh, s0, pl, kr, s0, np.zeros((2, 40, 40, 3))), dict(field_ptr=[0, 3, 2]), "must not decrease"),
                            ((sh, s0, pl, kr, s0, T), dict(cutout_size=0), "cutout_size"),
                            ((sh, s0, pl, kr, s0, T), dict(cutout_size=30.5), "cutout_size"),
                            ((sh, s0, pl, kr, s0, T), dict(radii=(0.0,)), "radii"),
                            ((sh, s0, pl, kr, s0, T), dict(radii=np.ones(9)), "at most 8 radii"),
                            ((sh, s0, pl, kr, s0, T), dict(subsample=10), "subsample")):
        with pytest.raises(ValueError, match=match):
            call(*args, **kw)
    with pytest.raises(TypeError, match="cutout_size"):
        E.Context.scene_aperture_fields(object(), sh, s0, pl, kr, s0, T)
    with pytest.raises(ValueError, match="places are needed"):
        E.Engine.infer_fields_measure_aper_data(object(), np.zeros((1, 81, 81, 6)), [[0, 0]], [0, 1], None)
    with pytest.raises(ValueError, match="places are needed"):
        E.Engine.infer_fields_measure_aper_data(object(), np.zeros((1, 81, 81, 6)), [[0, 0]], [0, 1], None, return_fields=False)
    with pytest.raises(ValueError, match="radii"):
        E.Engine.infer_fields_measure_aper_data(object(), np.zeros((1, 81, 81, 6)), [[0, 0]], [0, 1], [[0, 0]], radii=(-2.0,))
    # the pointers of outputs without rows go as null
    out, ptrs = E._aperture_field_out(4, 6, E.aperture_params(radii=(), fractions=()))
    assert [p is None for p in ptrs] == [True, True, True, False, False, False]
    assert out["ap_model_sum"].shape == (4, 0, 6) and out["auto_field_area"].shape == (4,)
    out, ptrs = E._aperture_field_out(4, 6, E.aperture_params())
    assert list(out) == list(E.APERTURE_FIELD_KEYS) == list(afo.KEYS) and not any(p is None for p in ptrs)
    # an empty call returns without the library
    empty = E.Context.scene_aperture_fields(object(), sh[:0], s0[:0], pl[:0], kr[:0], s0[:0], T, cutout_size=31, radii=(3.0, 5.0))
    assert empty["ap_model_sum"].shape == (0, 2, 3) and empty["auto_field_area"].shape == (0,)


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
             "dv_aperture_params*": C.POINTER(_lib.DvApertureParams)}
    for name, nargs in (("dv_scene_aperture_fields", 21), ("dv_infer_fields_measure_aper_data", 36)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header, re.S)
        assert m, f"{name} is not declared in include/debvader_hip.h"
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)         # bound: the library exports it
        restype, argtypes = _lib.SIGNATURES[name]
        want = [ctype[t] for t in _c_types(m.group(1))]
        assert restype is C.c_int and len(argtypes) == len(want) == nargs
        for i, (a, w) in enumerate(zip(argtypes, want)):
            assert a is w, (name, i, a, w)
        assert getattr(_lib.lib, name).argtypes == argtypes
    # dv_infer_fields_measure_aper's arguments, then the six outputs
    assert _lib.SIGNATURES["dv_infer_fields_measure_aper_data"][1][:30] == _lib.SIGNATURES["dv_infer_fields_measure_aper"][1]
    assert _lib.SIGNATURES["dv_infer_fields_measure_aper_data"][1][30:] == _lib.SIGNATURES["dv_scene_aperture_fields"][1][15:]
    # every existing entry point keeps its signature
    for name, nargs in (("dv_infer_fields_measure_blend", 22), ("dv_infer_fields_measure_aper", 30), ("dv_scene_aperture", 19),
                        ("dv_scene_blend", 16)):
        assert len(_lib.SIGNATURES[name][1]) == nargs
    kernel = open(os.path.join(ROOT, "debvader_amd", "csrc", "aperture.hip")).read()
    assert "aperture_field_kernel" in kernel and "getenv" not in kernel and "atomic" not in kernel.replace("No atomics", "")
    engine = open(os.path.join(ROOT, "debvader_amd", "csrc", "engine.hip")).read()
    assert "launch_aperture_field(" in engine and "struct MeanFieldStage" in engine
