"""CPU checks of the aperture photometry: the numpy restatement of the definition on inputs whose answer
is known, the Python layer - debvader_amd.measure.measurement.measure_apertures / aperture_records and
DeblendFieldBatch.deblend_fields(measure=True, apertures=...) - over the stand-in engine of tests/stub_aperture_engine.py, and
the ABI.  No GPU is touched."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests import aperture_oracle as ao
from tests import measure_oracle as mo
from tests.stub_aperture_engine import CS, NB, Net, OracleContext, stub_aperture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MOMENTS = [(4.0, 0.0, 4.0), (6.0, 1.5, 3.0), (9.0, -2.0, 5.0), (2.25, 0.3, 1.8), (16.0, 3.0, 9.0)]
OFFSETS = [(-0.371, -0.001), (0.101, -0.471), (-0.352, 0.428)]
FRACTIONS = (0.2, 0.5, 0.8)


def _gaussian_rows():
    """every (moments, offset) of the family measured once: (M, offset, stamp, catalogue row, aperture row)"""
    rows = []
    for M in MOMENTS:
        for off in OFFSETS:
            I = mo.gaussian_stamp(31, M, off)
            sh, _, st = mo.adaptive_moments(I)
            assert st == 0
            rows.append((M, off, I, sh, ao.aperture_row(I[:, :, None] * np.ones(3), None, sh, st, 2, ao.params(radii=()), True)))
    return rows


GAUSSIAN_ROWS = _gaussian_rows()


def test_gaussians_give_the_closed_forms():
    """(a): a noise-free elliptical Gaussian in the ellipse of its own moments has the Kron radius sqrt(pi / 2), kron_min
    decides the automatic aperture, which then holds 1 - exp(-3.5^2 / 2) of the flux, and the flux radii follow from the
    same integral.  The error is pixelisation.  Measured with this restatement over the 15 cases: Kron radius within 3.64e-3,
    flux ratio within 7.85e-4, flux radii within 2.83e-2 relative (the 1.4-px galaxy (2.25, 0.3, 1.8)); the two galaxies of
    sigma >= 2.5 px, (9, -2, 5) and (16, 3, 9), stay within 6.25e-4, 2.29e-4 and 1.01e-2.  Asserted at 1.5 x."""
    r1_true, enc, rho_true = ao.gaussian_truth(FRACTIONS)
    worst = np.zeros(3)
    worst_wide = np.zeros(3)
    for M, off, I, sh, row in GAUSSIAN_ROWS:
        assert row["status"] == ao.OK and row["flags"] & ao.FLAG_KRON_MIN and row["kron"][1] == 3.5
        assert not row["flags"] & ao.FLAG_AUTO
        err = np.array([abs(row["kron"][0] - r1_true), abs(row["flux_auto"][2] / I.sum() - enc),
                        np.max(np.abs(row["flux_rho"] / rho_true - 1.0))])
        worst = np.maximum(worst, err)
        if M in ((9.0, -2.0, 5.0), (16.0, 3.0, 9.0)):
            worst_wide = np.maximum(worst_wide, err)
    print("closed forms, worst (kron, flux ratio, flux radii):", worst, "sigma >= 2.5 px:", worst_wide)
    assert worst[0] <= 1.5 * 3.64e-3 and worst[1] <= 1.5 * 7.85e-4 and worst[2] <= 1.5 * 2.83e-2
    assert worst_wide[0] <= 1.5 * 6.25e-4 and worst_wide[1] <= 1.5 * 2.29e-4 and worst_wide[2] <= 1.5 * 1.01e-2


def test_constant_stamp_gives_the_area():
    """(b): on a stamp of ones the flux of a circle is its area, exactly, and the area is pi R^2 to the pixelisation error of
    5 x 5 sub-pixels.  Measured with this restatement over the three offsets: 6.9e-3 at R = 2, 3.5e-3 at R = 4, 7.1e-4 at
    R = 8.  Asserted at 1.5 x."""
    P = np.ones((31, 31, 3))
    for R, measured in ((2.0, 6.9e-3), (4.0, 3.5e-3), (8.0, 7.1e-4)):
        worst = 0.0
        for off in OFFSETS:
            row = ao.aperture_row(P, P, (15.0 + off[0], 15.0 + off[1], 4.0, 0.0, 4.0), 0, 2, ao.params(radii=(R,), fractions=()))
            assert np.all(row["ap_flux"][0] == row["ap_area"][0]) and np.all(row["ap_var"][0] == row["ap_area"][0])
            assert row["flags"] & 0xff == 0
            worst = max(worst, abs(row["ap_area"][0] / (np.pi * R * R) - 1.0))
        print("R", R, "area error", worst)
        assert worst <= 1.5 * measured


def test_whole_pixel_apertures_with_one_sub_pixel():
    """(c): subsample = 1 tests the pixel centre alone"""
    rng = np.random.default_rng(5)
    P = rng.uniform(0.5, 1.5, size=(21, 21, 3))
    r0, c0, R = 10.3, 9.6, 4.0
    row = ao.aperture_row(P, None, (r0, c0, 4.0, 0.5, 3.0), 0, 2, ao.params(radii=(R,), subsample=1))
    r, c = np.mgrid[0:21, 0:21]
    inside = (r - r0) ** 2 + (c - c0) ** 2 <= R * R
    assert row["ap_area"][0] == inside.sum()
    assert np.allclose(row["ap_flux"][0], P[inside].sum(axis=0), rtol=1e-13, atol=0)


def test_shortcut_and_full_count_agree_on_every_pixel():
    """(c): the centre test decides a pixel only where all of its sub-pixels agree with it"""
    tested = 0
    for M, off, I, sh, row in GAUSSIAN_ROWS[::2]:
        r0, c0, Mrr, Mrc, Mcc = sh
        det = Mrr * Mcc - Mrc * Mrc
        forms = [((1.0, 0.0, 1.0), rho) for rho in (0.3, 2.0, 3.0, 7.9)]
        forms += [((Mcc / det, (-2.0 * Mrc) / det, Mrr / det), rho) for rho in (0.05, 0.7, 1.0, 2.2, 3.5, 6.0)]
        for s in (1, 2, 5, 9):
            for form, rho in forms:
                full, _ = ao.counts(31, r0, c0, form, rho, s, shortcut=False)
                short, _ = ao.counts(31, r0, c0, form, rho, s, shortcut=True)
                assert np.array_equal(full, short), (M, off, s, form, rho)
                tested += 1
    assert tested == 8 * 4 * 10
    # and through a whole row, bisection included
    M, off, I, sh, row = GAUSSIAN_ROWS[4]
    full = ao.aperture_row(I[:, :, None] * np.ones(3), None, sh, 0, 2, ao.params(radii=()), False)
    assert np.array_equal(full["flux_rho"], row["flux_rho"]) and np.array_equal(full["kron"], row["kron"])
    assert np.array_equal(full["flux_auto"], row["flux_auto"]) and full["decisions"] == row["decisions"]
    assert full["margin_sub"] <= row["margin_sub"]


def test_flags_of_a_blob_near_an_edge():
    """(c): a blob 4 px from the lower row edge: the 8-px circle leaves the stamp, the 3-px circle does not"""
    cs = 31
    I = mo.gaussian_stamp(cs, (2.0, 0.0, 2.0), (-11.0, 0.0))        # centred at row 4
    sh = (4.0, 15.0, 2.0, 0.0, 2.0)
    row = ao.aperture_row(I[:, :, None] * np.ones(3), None, sh, 0, 2, ao.params(radii=(3.0, 8.0)))
    assert row["flags"] & 0xff == 0b10
    # rho_auto sqrt(2) = 4.95 > 4.5 and 6 sqrt(2) = 8.5: both ellipses leave it; kron_min decides
    assert row["flags"] & ao.FLAG_AUTO and row["flags"] & ao.FLAG_LIMIT and row["flags"] & ao.FLAG_KRON_MIN
    assert row["status"] == ao.OK and row["ap_area"][1] < np.pi * 64.0 * 0.85       # truncated, not an error
    I = mo.gaussian_stamp(cs, (2.0, 0.0, 2.0), (0.0, 0.0))
    centred = ao.aperture_row(I[:, :, None] * np.ones(3), None, (15.0, 15.0, 2.0, 0.0, 2.0), 0, 2, ao.params(radii=(3.0, 8.0)))
    assert centred["flags"] & 0x3ff == 0


def test_status_4_and_7():
    """(c): rows that cannot be used, and a plane without light inside the kron_limit ellipse"""
    I = mo.gaussian_stamp(31, (4.0, 0.0, 4.0), (0.2, 0.1))
    P = I[:, :, None] * np.ones(3)
    good = (15.2, 15.1, 4.0, 0.0, 4.0)
    for sh, st in (((np.nan,) + good[1:], 0), (good, 3), (good, 1), ((15.0, 15.0, 1e-3, 0.0, 1e-4), 0), (good[:4] + (np.inf,), 0)):
        row = ao.aperture_row(P, P, sh, st, 2, ao.params())
        assert row["status"] == ao.INELIGIBLE and row["flags"] == 0
        for k in ("ap_flux", "ap_flux_err", "ap_area", "flux_auto", "flux_auto_err", "kron", "flux_rho"):
            assert np.all(np.isnan(row[k])), k
    assert ao.aperture_row(P, P, good, 2, 2, ao.params())["status"] == ao.OK          # the iteration limit is eligible
    r, c = np.mgrid[0:31, 0:31]
    hole = P.copy()
    hole[(r - 15.2) ** 2 + (c - 15.1) ** 2 <= 13.0 ** 2] = 0.0                    # the kron_limit ellipse has the radius 12
    row = ao.aperture_row(hole, hole, good, 0, 2, ao.params())
    assert row["status"] == ao.NO_KRON
    for k in ("flux_auto", "flux_auto_err", "kron", "flux_rho"):
        assert np.all(np.isnan(row[k])), k
    assert np.all(row["ap_flux"] == 0.0) and np.all(row["ap_area"] > 0.0) and np.all(row["ap_flux_err"] == 0.0)
    negative = ao.aperture_row(-P, None, good, 0, 2, ao.params())
    assert negative["status"] == ao.NO_KRON and np.all(negative["ap_flux"] < 0.0)


# ---- (d) the host layer over the stand-in engine -----------------------------------------------------------------------------

def test_aperture_records_columns_and_derived_values():
    from debvader_amd.measure import measurement as ms

    names = [c[0] for c in ms.aperture_dtype(6, 3, 3)]
    assert names == ["ap_flux", "ap_flux_err", "ap_area", "flux_auto", "flux_auto_err", "kron_radius", "rho_auto", "auto_area",
                     "flux_rho", "aper_flags", "aper_status", "flux_radius", "kron_a", "kron_b", "concentration"]
    dt = np.dtype(ms.aperture_dtype(6, 3, 2))
    assert dt["ap_flux"].shape == (3, 6) and dt["ap_area"].shape == (3,) and dt["flux_rho"].shape == (2,)
    assert dt["flux_radius"].shape == (2,) and dt["aper_flags"] == np.int32
    n, nb, K, J = 6, 6, 3, 3
    s = stub_aperture(n, nb, K, J)
    shape = np.stack([np.full(n, 29.0), np.full(n, 29.0), 4.0 + np.arange(n), np.full(n, 0.5), 9.0 + np.arange(n)], axis=1)
    rec = ms.aperture_records(*(s[k] for k in ("ap_flux", "ap_flux_err", "ap_area", "flux_auto", "flux_auto_err", "kron",
                                               "flux_rho", "aper_flags", "aper_status")), shape)
    assert rec["aper_status"].tolist() == [0, 7, 0, 0, 4, 0]
    for k in ("ap_flux", "ap_flux_err", "ap_area", "flux_auto", "flux_auto_err", "flux_rho"):
        assert np.array_equal(rec[k], s[k], equal_nan=True), k
    assert np.array_equal(rec["kron_radius"], s["kron"][:, 0], equal_nan=True)
    assert np.array_equal(rec["rho_auto"], s["kron"][:, 1], equal_nan=True)
    assert np.array_equal(rec["auto_area"], s["kron"][:, 2], equal_nan=True)
    for i in (0, 2, 3, 5):
        Mrr, Mrc, Mcc = shape[i, 2:]
        det = Mrr * Mcc - Mrc * Mrc
        lam = np.linalg.eigvalsh(np.array([[Mrr, Mrc], [Mrc, Mcc]]))
        assert np.allclose(rec["flux_radius"][i], s["flux_rho"][i] * det ** 0.25, rtol=1e-15)
        assert np.isclose(rec["kron_a"][i], s["kron"][i, 1] * np.sqrt(lam[1]), rtol=1e-13)
        assert np.isclose(rec["kron_b"][i], s["kron"][i, 1] * np.sqrt(lam[0]), rtol=1e-13)
        assert np.isclose(rec["concentration"][i], 5.0 * np.log10(3.0), rtol=1e-13)       # flux_rho[2] / flux_rho[0] = 3
        # the area of the automatic ellipse is pi a b
        assert np.isclose(rec["kron_a"][i] * rec["kron_b"][i], s["kron"][i, 1] ** 2 * np.sqrt(det), rtol=1e-13)
    for i in (1, 4):                                                            # NaN follows the GPU's
        for k in ("flux_radius", "kron_a", "kron_b", "concentration", "kron_radius", "flux_auto"):
            assert np.all(np.isnan(rec[k][i])), (i, k)
    assert not np.any(np.isnan(rec["ap_flux"][1])) and np.all(np.isnan(rec["ap_flux"][4]))
    # without a stddev stamp the error columns are NaN; one fraction has no concentration; no radii, no fractions
    s1 = stub_aperture(n, nb, K, 1)
    rec1 = ms.aperture_records(s1["ap_flux"], None, s1["ap_area"], s1["flux_auto"], None, s1["kron"], s1["flux_rho"],
                               s1["aper_flags"], s1["aper_status"], shape)
    assert np.all(np.isnan(rec1["ap_flux_err"])) and np.all(np.isnan(rec1["flux_auto_err"]))
    assert np.all(np.isnan(rec1["concentration"])) and rec1["flux_radius"].shape == (n, 1)
    s0 = stub_aperture(n, nb, 0, 0)
    rec0 = ms.aperture_records(*(s0[k] for k in ("ap_flux", "ap_flux_err", "ap_area", "flux_auto", "flux_auto_err", "kron",
                                                 "flux_rho", "aper_flags", "aper_status")), shape)
    assert rec0["ap_flux"].shape == (n, 0, nb) and rec0["ap_area"].shape == (n, 0) and rec0["flux_radius"].shape == (n, 0)
    assert np.array_equal(rec0["kron_a"], rec["kron_a"], equal_nan=True) and np.all(np.isnan(rec0["concentration"]))


def test_measure_apertures_measures_first_without_a_catalogue():
    from debvader_amd.measure import measurement as ms

    sig = inspect.signature(ms.measure_apertures).parameters
    assert list(sig)[:7] == ["mean", "stddev", "catalogue", "radii", "fractions", "band", "sigma0"]
    assert sig["radii"].default == (3.0, 5.0, 8.0) and sig["fractions"].default == (0.2, 0.5, 0.8) and sig["band"].default == 2
    ctx = OracleContext()
    stamps = np.stack([mo.gaussian_stamp(31, M, off)[:, :, None] * np.ones(3) for M, off in
                       (((4.0, 0.0, 4.0), (0.2, -0.3)), ((6.0, 1.5, 3.0), (-0.4, 0.1)))]).astype(np.float32)
    rec = ms.measure_apertures(stamps, ctx=ctx)
    assert [("n" in c, "aperture" in c) for c in ctx.calls] == [(True, False), (False, True)]
    assert ctx.calls[1]["radii"] == (3.0, 5.0, 8.0) and not ctx.calls[1]["with_stddev"]
    assert rec["aper_status"].tolist() == [0, 0] and np.all(np.isnan(rec["ap_flux_err"]))
    r1_true, enc, rho_true = ao.gaussian_truth(FRACTIONS)
    assert np.all(np.abs(rec["kron_radius"] - r1_true) < 1.5 * 3.64e-3)
    sigma = (np.array([16.0, 18.0 - 2.25])) ** 0.25
    assert np.all(np.abs(rec["flux_radius"] / (rho_true[None, :] * sigma[:, None]) - 1.0) < 1.5 * 2.83e-2)
    assert np.all(rec["concentration"] > 0) and np.all(rec["kron_a"] >= rec["kron_b"])
    cat = ms.measure_stamps(stamps, ctx=ctx)
    ctx.calls.clear()
    rec2 = ms.measure_apertures(stamps, 0.1 * stamps, catalogue=cat, radii=(), fractions=(0.5,), ctx=ctx)
    assert len(ctx.calls) == 1 and ctx.calls[0]["radii"] == () and ctx.calls[0]["with_stddev"]
    assert rec2["ap_flux"].shape == (2, 0, 3) and rec2["flux_rho"].shape == (2, 1)
    assert np.array_equal(rec2["flux_auto"], rec["flux_auto"]) and np.all(rec2["flux_auto_err"] > 0)
    assert np.array_equal(rec2["flux_rho"][:, 0], rec["flux_rho"][:, 1])


F = 81
DIST = [np.array([[0.0, 0.0], [5.0, -7.0]]), np.zeros((0, 2)), np.array([[100.0, 0.0], [-3.0, 11.0]]), np.array([[0.0, 40.0]])]


def _batch():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch

    net = Net()
    return net, DeblendFieldBatch(net, np.random.default_rng(3).normal(size=(4, F, F, NB)), CS, NB)


def test_deblend_fields_appends_the_aperture_columns():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch
    from debvader_amd.measure import measurement as ms
    from tests.stub_measure_engine import stub_catalogue

    sig = inspect.signature(DeblendFieldBatch.deblend_fields).parameters
    assert sig["apertures"].default is None and sig["flux_fractions"].default is None
    assert DeblendFieldBatch.aperture_columns(NB, 2, 3) == ms.aperture_dtype(NB, 2, 3)
    net, b = _batch()
    for apertures, fractions, K, J in (((3.0, 5.0, 8.0), None, 3, 3), ((), None, 0, 3), ((4.0,), (0.5,), 1, 1), ([2.0, 6.0], (), 2, 0)):
        want = np.dtype(DeblendFieldBatch.ON_DEVICE_COLUMNS + DeblendFieldBatch.measure_columns(NB) +
                        DeblendFieldBatch.aperture_columns(NB, K, J))
        for rf in (True, False):
            kw = {} if fractions is None else {"flux_fractions": fractions}
            res = b.deblend_fields(DIST, on_device=True, measure=True, apertures=apertures, return_fields=rf, **kw)
            call = net._core.engine.calls[-2]
            assert call[0] == "infer_fields_measure_aper" and call[2] is rf and (call[3] is None) == (not rf)
            assert call[4] == tuple(float(r) for r in apertures)
            assert call[5] == ((0.2, 0.5, 0.8) if fractions is None else tuple(fractions))
            assert [len(r) for r in res] == [2, 0, 1, 0] and all(r.dtype == want for r in res)
            s = stub_aperture(3, NB, K, J)
            cat = ms.aperture_records(*(s[k] for k in ("ap_flux", "ap_flux_err", "ap_area", "flux_auto", "flux_auto_err", "kron",
                                                       "flux_rho", "aper_flags", "aper_status")), stub_catalogue(3, NB)["shape"])
            for i, (m, k) in enumerate([(0, 0), (0, 1), (2, 0)]):
                for n in cat.dtype.names:
                    assert np.array_equal(res[m][n][k], cat[n][i], equal_nan=True), n
            assert res[0]["flux"][1, 0] == 1.0 and res[0]["aper_status"].tolist() == [0, 7]
    b.deblend_fields(DIST, on_device=True, measure=True)
    assert net._core.engine.calls[-2][0] == "infer_fields_measure"


def test_deblend_fields_refuses_aperture_combinations():
    net, b = _batch()
    for kw, match in ((dict(), "need measure=True and on_device=True"),
                      (dict(measure=True), "need measure=True and on_device=True"),
                      (dict(on_device=True), "need measure=True and on_device=True"),
                      (dict(on_device=True, measure=True, psf=np.ones((21, 21))), "cannot be combined with psf"),
                      (dict(on_device=True, measure=True, blendedness=True), "cannot be combined with blendedness"),
                      (dict(on_device=True, measure=True, measure_samples=4), "cannot be combined with measure_samples"),
                      (dict(on_device=True, measure=True, optimise_positions=True), "cannot be combined with optimise_positions"),
                      (dict(on_device=True, measure=True, epistemic_uncertainty_estimation=True),
                       "cannot be combined with epistemic_uncertainty_estimation")):
        with pytest.raises(ValueError, match=match):
            b.deblend_fields(DIST, apertures=(3.0, 5.0), **kw)
    with pytest.raises(ValueError, match="give apertures too"):
        b.deblend_fields(DIST, on_device=True, measure=True, flux_fractions=(0.5,))
    for kw, match in ((dict(apertures=(3.0, -1.0)), "radii must be finite and positive"),
                      (dict(apertures=(3.0, np.inf)), "radii must be finite and positive"),
                      (dict(apertures=tuple(range(1, 10))), "at most 8 radii"),
                      (dict(apertures=(), flux_fractions=(0.1, 0.2, 0.3, 0.4, 0.5)), "4 fractions"),
                      (dict(apertures=(), flux_fractions=(0.5, 1.0)), "strictly between 0 and 1"),
                      (dict(apertures=(), flux_fractions=(0.0,)), "strictly between 0 and 1")):
        with pytest.raises(ValueError, match=match):
            b.deblend_fields(DIST, on_device=True, measure=True, **kw)
    assert not [c for c in net._core.engine.calls if c[0].startswith("infer")]


def test_engine_wrappers_refuse_before_the_library():
    from debvader_amd import engine as E

    st = np.zeros((2, 31, 31, 3), np.float32)
    sh, s0 = np.zeros((2, 5)), np.zeros(2, np.int32)
    for kw, match in ((dict(radii=(0.0,)), "radii"), (dict(radii=(np.nan,)), "radii"), (dict(radii=np.ones(9)), "at most 8 radii"),
                      (dict(fractions=(1.5,)), "strictly between"), (dict(fractions=np.full(5, 0.5)), "4 fractions"),
                      (dict(subsample=0), "subsample"), (dict(subsample=10), "subsample"), (dict(subsample=2.5), "subsample"),
                      (dict(bisect_iters=0), "bisect_iters"), (dict(bisect_iters=61), "bisect_iters"),
                      (dict(kron_factor=0.0), "kron_factor"), (dict(kron_min=np.inf), "kron_min"),
                      (dict(kron_limit=-1.0), "kron_limit"), (dict(band=3), "band 3")):
        with pytest.raises(ValueError, match=match):
            E.Context.scene_aperture(object(), st, sh, s0, **kw)
    with pytest.raises(ValueError, match="at most 90"):
        E.Context.scene_aperture(object(), np.zeros((1, 91, 91, 3), np.float32), sh[:1], s0[:1])
    with pytest.raises(ValueError, match="expected shape"):
        E.Context.scene_aperture(object(), st, sh[:1], s0)
    with pytest.raises(ValueError, match="stddev stamps"):
        E.Context.scene_aperture(object(), st, sh, s0, stddev=st[:1])
    with pytest.raises(ValueError, match="places are needed"):
        E.Engine.infer_fields_measure_aper(object(), np.zeros((1, 81, 81, 6)), [[0, 0]], [0, 1])
    with pytest.raises(ValueError, match="radii"):
        E.Engine.infer_fields_measure_aper(object(), np.zeros((1, 81, 81, 6)), [[0, 0]], [0, 1], radii=(-2.0,), return_fields=False)
    par = E.aperture_params()
    assert (par.n_radii, par.n_fractions, par.subsample, par.bisect_iters) == (3, 3, 5, 32)
    assert list(par.radii)[:3] == [3.0, 5.0, 8.0] and list(par.fractions)[:3] == [0.2, 0.5, 0.8]
    assert (par.kron_factor, par.kron_min, par.kron_limit) == (2.5, 3.5, 6.0)
    # the pointers of outputs without rows go as null
    out, ptrs = E._aperture_out(4, 6, E.aperture_params(radii=(), fractions=()))
    assert [p is None for p in ptrs] == [True, True, True, False, False, False, True, False, False]
    assert out["ap_flux"].shape == (4, 0, 6) and out["flux_rho"].shape == (4, 0)
    out, ptrs = E._aperture_out(4, 6, E.aperture_params(), err=False)
    assert "ap_flux_err" not in out and [p is None for p in ptrs] == [False, True, False, False, True, False, False, False, False]


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
    for name, nargs in (("dv_aperture_params_default", 1), ("dv_scene_aperture", 19), ("dv_infer_fields_measure_aper", 30)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header, re.S)
        assert m, f"{name} is not declared in include/debvader_hip.h"
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)         # bound: the library exports it
        restype, argtypes = _lib.SIGNATURES[name]
        want = [ctype[t] for t in _c_types(m.group(1))]
        assert restype is C.c_int and len(argtypes) == len(want) == nargs
        for i, (a, w) in enumerate(zip(argtypes, want)):
            assert a is w, (name, i, a, w)
        assert getattr(_lib.lib, name).argtypes == argtypes
    assert _lib.SIGNATURES["dv_infer_fields_measure_aper"][1][:20] == _lib.SIGNATURES["dv_infer_fields_measure"][1]
    assert _lib.SIGNATURES["dv_infer_fields_measure_aper"][1][21:] == _lib.SIGNATURES["dv_scene_aperture"][1][10:]
    # the struct: the header's fields in the header's order, and the library's defaults through it
    body = re.search(r"typedef struct dv_aperture_params \{(.*?)\} dv_aperture_params;", header, re.S).group(1)
    fields = re.findall(r"(int32_t|double)\s+(\w+)(?:\[(\d+)\])?;", body)
    want = [(n, "int32_t" if t is C.c_int32 else "double", str(getattr(t, "_length_", "")))
            for n, t in _lib.DvApertureParams._fields_]
    assert [(n, t, d) for t, n, d in fields] == want
    assert C.sizeof(_lib.DvApertureParams) == 4 * 4 + 15 * 8
    par = _lib.DvApertureParams()
    assert _lib.lib.dv_aperture_params_default(par) == 0 and _lib.lib.dv_aperture_params_default(None) == -1
    assert (par.n_radii, par.n_fractions, par.subsample, par.bisect_iters) == (3, 3, 5, 32)
    assert list(par.radii) == [3.0, 5.0, 8.0, 0, 0, 0, 0, 0] and list(par.fractions) == [0.2, 0.5, 0.8, 0.0]
    assert (par.kron_factor, par.kron_min, par.kron_limit) == (2.5, 3.5, 6.0)
    src = open(os.path.join(ROOT, "debvader_amd", "csrc", "Makefile")).read()
    assert "aperture.hip" in src and os.path.exists(os.path.join(ROOT, "debvader_amd", "csrc", "aperture.hip"))
    kernel = open(os.path.join(ROOT, "debvader_amd", "csrc", "aperture.hip")).read()
    assert "getenv" not in kernel and "#pragma clang fp contract(off)" in kernel and "exp(" not in kernel
