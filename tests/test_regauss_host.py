"""CPU checks of the PSF correction: the numpy restatement of the definition on inputs whose answer is
known, the Python layer - debvader_amd.measure.measurement.measure_stamps_psf / psf_records and
DeblendFieldBatch.deblend_fields(measure=True, psf=...) - over the stand-in engine of tests/stub_regauss_engine.py, and the
ABI.  No GPU is touched."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests import measure_oracle as mo
from tests import regauss_oracle as ro
from tests.stub_regauss_engine import CS, NB, Net, OracleContext, stub_regauss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _shapes(M):
    tr = M[0] + M[2]
    return np.array([(M[2] - M[0]) / tr, 2.0 * M[1] / tr]), (M[0] * M[2] - M[1] * M[1]) ** 0.25


def test_iteration_with_a_start_state_is_the_measurement_oracles():
    I = mo.gaussian_stamp(31, (5.0, 1.0, 7.0), (0.6, -1.2)) + 0.01
    ctr = 15.0
    for s0 in (2.0, 3.0):
        a = mo.adaptive_moments(I, s0)
        b = ro.adaptive_moments_from(I, (ctr, ctr, s0 * s0, 0.0, s0 * s0))
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
    # a start at the answer converges at once and stays there
    b2 = ro.adaptive_moments_from(I, b[0])
    assert b2[2] == 0 and b2[1] <= 2 and np.allclose(b2[0], b[0], rtol=0, atol=1e-9)


def test_gaussian_galaxy_gaussian_psf_is_recovered():
    """(a): eps vanishes, I' = I, and M' - M_P is the galaxy's own covariance"""
    cs, ps = 41, 21
    Cf, CP = np.array([5.0, 1.2, 7.5]), np.array([2.2, -0.3, 1.8])
    off = (0.8, -0.45)
    I = ro.norm_gaussian(cs, Cf + CP, off, 50.0)
    Q = ro.norm_gaussian(ps, CP, (0.3, -0.2))
    row, it, st = mo.adaptive_moments(I)
    P = ro.psf_row(Q)
    assert st == 0 and P["status"] == 0 and P["usable"]
    # (a Gaussian sampled at the pixel centres is its own best Gaussian up to the aliasing of the sampling, e^(-2 pi^2 M / 2)
    # = 2e-8 of the peak for the narrow axis of the weighted image here)
    assert np.abs(P["eps"]).max() < 1e-6 * P["aux"][0]
    out, it2, st2 = ro.regauss_one(I, row, st, P)
    Mg = out[2:5] - P["shape"][2:5]
    print("M_g - C_f", Mg - Cf, "rho4", out[5], P["aux"][2], "centroid", out[:2] - row[:2], "iters", it2)
    assert st2 == 0
    assert np.abs(Mg - Cf).max() <= 1e-6 * (Cf[0] + Cf[2])
    assert abs(out[5] - 2.0) < 1e-4 and abs(P["aux"][2] - 2.0) < 1e-4
    assert np.abs(out[:2] - row[:2]).max() < 1e-5
    assert abs(out[0] - (20.0 + off[0])) < 1e-5 and abs(out[1] - (20.0 + off[1])) < 1e-5
    # A_P is the peak of the normalised Gaussian, FQ its flux
    assert P["aux"][0] == pytest.approx(1.0 / (2 * np.pi * np.sqrt(CP[0] * CP[2] - CP[1] ** 2)), rel=1e-6)
    assert P["aux"][1] == pytest.approx(1.0, abs=1e-6)


def test_double_gaussian_psf_is_corrected_five_times_better_than_by_subtraction():
    """(b): twelve seeded cases; the re-Gaussianized shapes against the plain subtraction M_I - M_P"""
    worst_e = worst_s = 0.0
    tot = np.zeros(4)
    for seed in range(12):
        stamp, psf, Cf = ro.double_gaussian_case(seed)
        row, it, st = mo.adaptive_moments(stamp)
        P = ro.psf_row(psf)
        out, it2, st2 = ro.regauss_one(stamp, row, st, P)
        assert (st, P["status"], st2) == (0, 0, 0)
        d = ro.derived(out[None], [st2], [P["shape"]], [0])
        e_true, s_true = _shapes(Cf)
        e_unc, s_unc = _shapes(row[2:5] - P["shape"][2:5])
        err = np.array([max(abs(d["e1_corr"][0] - e_true[0]), abs(d["e2_corr"][0] - e_true[1])), np.abs(e_unc - e_true).max(),
                        abs(d["sigma_corr"][0] / s_true - 1.0), abs(s_unc / s_true - 1.0)])
        print(f"seed {seed:2d}: e {err[0]:.2e} against {err[1]:.2e}, sigma {err[2]:.2e} against {err[3]:.2e}, iters {it2}, "
              f"rho4 {out[5]:.4f}, psf_rho4 {P['aux'][2]:.4f}, resolution {d['resolution'][0]:.3f}")
        assert err[0] <= 0.2 * err[1] and err[2] <= 0.2 * err[3]
        worst_e, worst_s = max(worst_e, err[0] / err[1]), max(worst_s, err[2] / err[3])
        tot = np.maximum(tot, err)
    print(f"worst ratios: e {worst_e:.3f}, sigma {worst_s:.3f}; maxima {tot}")
    assert tot[0] <= 0.2 * tot[1] and tot[2] <= 0.2 * tot[3]


def test_statuses_and_their_nan_rows():
    """(c)"""
    cs, ps = 31, 15
    good = ro.norm_gaussian(cs, np.array([6.0, 0.5, 5.0]), (0.2, 0.3), 10.0)
    narrow = ro.norm_gaussian(cs, np.array([1.5, 0.0, 1.5]), (0.0, 0.0), 10.0)
    psf = np.stack([ro.norm_gaussian(ps, np.array([2.5, 0.1, 2.0]), (0.1, 0.0)), np.zeros((ps, ps))])
    stamps = np.stack([good, np.zeros((cs, cs)), good, good, good, narrow, good])[:, :, :, None] * np.ones(3)
    cat = mo.measure(stamps, None, 1)
    assert cat["status"].tolist() == [0, 3, 0, 0, 0, 0, 0]
    index = [0, 0, 1, -1, 2, 0, 0]
    shape = cat["shape"].copy()
    shape[6, 3] = np.nan
    out = ro.regauss(stamps, shape, cat["status"], index, psf, band=1)
    assert out["regauss_status"].tolist() == [0, 4, 5, 5, 5, 6, 4]
    assert out["psf_status"].tolist() == [0, 3] and np.isnan(out["psf_aux"][1, 0]) and out["psf_aux"][1, 1] == 0.0
    for i in range(1, 7):
        assert np.isnan(out["regauss"][i]).all() and out["regauss_iters"][i] == 0
    assert np.isfinite(out["regauss"][0]).all() and out["regauss_iters"][0] > 0
    d = ro.derived(out["regauss"], out["regauss_status"], out["psf_shape"], index)
    assert np.isfinite(d["sigma_corr"][0]) and all(np.isnan(d[k][1:]).all() for k in d)


# ---- the host layer -----------------------------------------------------------------------------------------------------------
def test_psf_records_columns_values_and_nan_rules():
    from debvader_amd.measure import measurement as ms

    names = [c[0] for c in ms.psf_dtype()]
    assert names == ["regauss_row", "regauss_col", "regauss_Mrr", "regauss_Mrc", "regauss_Mcc", "rho4", "regauss_iters",
                     "regauss_status", "psf_index", "psf_Mrr", "psf_Mrc", "psf_Mcc", "psf_rho4", "sigma_corr", "e1_corr",
                     "e2_corr", "resolution"]
    assert (ms.STATUS_INELIGIBLE, ms.STATUS_NO_PSF, ms.STATUS_UNRESOLVED) == (4, 5, 6)
    s = stub_regauss(8, 2)
    rg, st = s["regauss"].copy(), s["regauss_status"].copy()
    st[1] = 3                                            # a failed iteration keeps its state, the derived values are NaN
    rg[2, 2:5] = [2.5, 0.25, 2.9]                        # M' - M_P has a negative determinant: shapes NaN, resolution kept
    index = np.array([0, 1, 0, 0, 1, 7, -1, 0])
    rec = ms.psf_records(rg, s["regauss_iters"], st, s["psf_shape"], s["psf_aux"], index)
    assert rec.dtype == np.dtype(ms.psf_dtype()) and len(rec) == 8
    want = ro.derived(rg, st, s["psf_shape"], index)
    for k in ("sigma_corr", "e1_corr", "e2_corr", "resolution"):
        assert np.array_equal(np.isnan(rec[k]), np.isnan(want[k])), k
        assert np.allclose(rec[k], want[k], rtol=1e-14, atol=0, equal_nan=True), k
    # row 0: M' = (9, .5, 12), M_P = (2, .25, 3)
    G = np.array([7.0, 0.25, 9.0])
    assert rec["sigma_corr"][0] == pytest.approx((63.0 - 0.0625) ** 0.25) and rec["e1_corr"][0] == pytest.approx(2.0 / 16.0)
    assert rec["e2_corr"][0] == pytest.approx(0.5 / 16.0) and rec["resolution"][0] == pytest.approx(1.0 - 5.0 / 21.0)
    assert np.isnan(rec["sigma_corr"][[1, 2, 3, 5, 6, 7]]).all() and np.isfinite(rec["sigma_corr"][[0, 4]]).all()
    assert np.isfinite(rec["resolution"][2]) and np.isnan(rec["resolution"][1])
    assert rec["psf_Mrr"].tolist()[:5] == [2.0, 3.0, 2.0, 2.0, 3.0] and np.isnan(rec["psf_Mrr"][5:7]).all()
    assert rec["psf_Mcc"][1] == 4.0 and rec["psf_Mrc"][0] == 0.25 and rec["psf_rho4"][1] == s["psf_aux"][1, 2]
    assert rec["psf_index"].tolist() == index.tolist() and rec["rho4"][0] == 2.0 and rec["regauss_iters"][0] == 30
    assert G[0] == rec["regauss_Mrr"][0] - rec["psf_Mrr"][0]


def test_measure_stamps_psf_measures_first_or_takes_a_catalogue():
    from debvader_amd.measure import measurement as ms

    stamps = np.stack([ro.double_gaussian_case(s)[0] for s in (0, 1)])[:, :, :, None].astype(np.float32) * np.ones(3, np.float32)
    psf = np.stack([ro.double_gaussian_case(s)[1] for s in (0, 1)])
    ctx = OracleContext()
    rec = ms.measure_stamps_psf(stamps, psf, [0, 1], ctx=ctx)
    assert [("regauss" in c) for c in ctx.calls] == [False, True] and not ctx.calls[0]["with_stddev"]
    assert ctx.calls[1]["index"].tolist() == [0, 1] and ctx.calls[1]["K"] == 2 and ctx.calls[1]["psf_sigma0"] == 2.0
    assert rec["regauss_status"].tolist() == [0, 0]
    for s in (0, 1):
        e_true, s_true = _shapes(ro.double_gaussian_case(s)[2])
        assert abs(rec["e1_corr"][s] - e_true[0]) < 2e-3 and abs(rec["sigma_corr"][s] / s_true - 1) < 5e-3
    cat = ms.measure_stamps(stamps, ctx=ctx)
    ctx.calls.clear()
    rec2 = ms.measure_stamps_psf(stamps, psf[0], catalogue=cat, ctx=ctx)     # one image for all
    assert len(ctx.calls) == 1 and ctx.calls[0]["index"].tolist() == [0, 0] and ctx.calls[0]["K"] == 1
    assert rec2["sigma_corr"][0] == rec["sigma_corr"][0] and rec2["psf_index"].tolist() == [0, 0]
    with pytest.raises(ValueError, match="psf_index"):
        ms.measure_stamps_psf(stamps, psf, [0, 1, 0], ctx=ctx)
    with pytest.raises(ValueError, match="PSF images"):
        ms.measure_stamps_psf(stamps, np.zeros((1, 4, 4)), ctx=ctx)
    with pytest.raises(ValueError, match="PSF images"):
        ms.measure_stamps_psf(stamps, np.zeros((1, 35, 35)), ctx=ctx)
    with pytest.raises(ValueError, match="psf_sigma0"):
        ms.measure_stamps_psf(stamps, psf, psf_sigma0=0.0, ctx=ctx)


F = 81
DIST = [np.array([[0.0, 0.0], [5.0, -7.0]]), np.zeros((0, 2)), np.array([[100.0, 0.0], [-3.0, 11.0]]), np.array([[0.0, 40.0]])]


def _batch():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch

    net = Net()
    return net, DeblendFieldBatch(net, np.random.default_rng(3).normal(size=(4, F, F, NB)), CS, NB)


def test_deblend_fields_psf_forms_and_their_indices():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch
    from debvader_amd.measure import measurement as ms

    sig = inspect.signature(DeblendFieldBatch.deblend_fields).parameters
    assert sig["psf"].default is None and sig["psf_index"].default is None
    assert DeblendFieldBatch.psf_columns() == ms.psf_dtype()
    net, b = _batch()
    one = np.ones((21, 21))
    want = np.dtype(DeblendFieldBatch.ON_DEVICE_COLUMNS + DeblendFieldBatch.measure_columns(NB) + DeblendFieldBatch.psf_columns())
    for psf, psf_index, K, index in ((one, None, 1, [0, 0, 0]),                            # one for all
                                     (np.stack([one * k for k in range(4)]), None, 4, [0, 0, 2]),      # one per field
                                     (np.stack([one, 2 * one]), [1, 0, 1], 2, [1, 0, 1]),             # per galaxy, flat
                                     (np.stack([one, 2 * one]), [[1, 1], [], [0], []], 2, [1, 1, 0])):  # per galaxy, per field
        for rf in (True, False):
            res = b.deblend_fields(DIST, on_device=True, measure=True, psf=psf, psf_index=psf_index, return_fields=rf)
            call = net._core.engine.calls[-2]
            assert call[0] == "infer_fields_measure_psf" and call[2] is rf and (call[3] is None) == (not rf)
            assert call[4].shape == (K, 21, 21) and call[5].tolist() == index
            assert [len(r) for r in res] == [2, 0, 1, 0] and all(r.dtype == want for r in res)
            s = stub_regauss(3, K)
            cat = ms.psf_records(s["regauss"], s["regauss_iters"], s["regauss_status"], s["psf_shape"], s["psf_aux"], index)
            for i, (m, k) in enumerate([(0, 0), (0, 1), (2, 0)]):
                for n in cat.dtype.names:
                    assert np.array_equal(res[m][n][k], cat[n][i], equal_nan=True), n
            assert res[0]["psf_index"].tolist() == index[:2] and res[0]["flux"][1, 0] == 1.0
            assert sorted(b.psf_moments) == ["psf_aux", "psf_iters", "psf_shape", "psf_status"]
            assert b.psf_moments["psf_shape"].shape == (K, 5)
    b.deblend_fields(DIST, on_device=True, measure=True)
    assert b.psf_moments is None and net._core.engine.calls[-2][0] == "infer_fields_measure"


def test_deblend_fields_refuses_psf_combinations():
    net, b = _batch()
    one = np.ones((21, 21))
    for kw, match in ((dict(), "needs measure=True and on_device=True"),
                      (dict(measure=True), "needs measure=True and on_device=True"),
                      (dict(on_device=True), "needs measure=True and on_device=True"),
                      (dict(on_device=True, measure=True, blendedness=True), "cannot be combined with blendedness"),
                      (dict(on_device=True, measure=True, measure_samples=4), "cannot be combined with measure_samples"),
                      (dict(on_device=True, measure=True, optimise_positions=True), "cannot be combined with optimise_positions"),
                      (dict(on_device=True, measure=True, epistemic_uncertainty_estimation=True),
                       "cannot be combined with epistemic_uncertainty_estimation")):
        with pytest.raises(ValueError, match=match):
            b.deblend_fields(DIST, psf=one, **kw)
    with pytest.raises(ValueError, match="give psf too"):
        b.deblend_fields(DIST, on_device=True, measure=True, psf_index=[0, 0, 0])
    with pytest.raises(ValueError, match="one PSF per field"):
        b.deblend_fields(DIST, on_device=True, measure=True, psf=np.ones((3, 21, 21)))
    with pytest.raises(ValueError, match="one integer per deblended galaxy"):
        b.deblend_fields(DIST, on_device=True, measure=True, psf=np.ones((3, 21, 21)), psf_index=[0, 1])
    with pytest.raises(ValueError, match="serves every galaxy"):
        b.deblend_fields(DIST, on_device=True, measure=True, psf=one, psf_index=[0, 0, 0])
    with pytest.raises(ValueError, match="PSF image"):
        b.deblend_fields(DIST, on_device=True, measure=True, psf=np.ones(21))
    assert not [c for c in net._core.engine.calls if c[0].startswith("infer")]


def test_engine_wrappers_refuse_before_the_library():
    from debvader_amd import engine as E

    st = np.zeros((2, 31, 31, 3), np.float32)
    sh, s0 = np.zeros((2, 5)), np.zeros(2, np.int32)
    for kw, match in ((dict(psf=np.ones((1, 4, 4))), "PSF images of 4 pixels"), (dict(psf=np.ones((2, 9, 7))), "square PSF"),
                      (dict(psf=np.ones((1, 9, 9)), psf_sigma0=np.nan), "psf_sigma0"),
                      (dict(psf=np.ones((1, 9, 9)), psf_index=[0.5, 1.0]), "integers"),
                      (dict(psf=np.ones((1, 9, 9)), band=3), "band 3"), (dict(psf=np.ones((1, 9, 9)), tol=0.0), "tol")):
        with pytest.raises(ValueError, match=match):
            E.Context.scene_regauss(object(), st, sh, s0, **kw)
    with pytest.raises(ValueError, match="at most 64"):
        E.Context.scene_regauss(object(), np.zeros((1, 65, 65, 3), np.float32), sh[:1], s0[:1], np.ones((9, 9)))
    with pytest.raises(ValueError, match="expected shape"):
        E.Context.scene_regauss(object(), st, sh[:1], s0, np.ones((9, 9)))
    with pytest.raises(ValueError, match="places are needed"):
        E.Engine.infer_fields_measure_psf(object(), np.zeros((1, 81, 81, 6)), [[0, 0]], [0, 1], np.ones((9, 9)))
    with pytest.raises(ValueError, match="PSF images of 3 pixels"):
        E.Engine.infer_fields_measure_psf(object(), np.zeros((1, 81, 81, 6)), [[0, 0]], [0, 1], np.ones((3, 3)), return_fields=False)
    # an index out of range is a row status, not an error; a huge one stays out of range after the cast
    psf, index = E.check_psf_args(np.ones((9, 9)), np.array([-5, 0, 2 ** 40]), 3, 2.0)
    assert psf.shape == (1, 9, 9) and index.dtype == np.int32 and index[0] < 0 and index[1] == 0 and index[2] >= 1


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
             "uint64_t": C.c_uint64, "double": C.c_double, "dv_measure_params*": C.POINTER(_lib.DvMeasureParams)}
    for name, nargs in (("dv_scene_regauss", 22), ("dv_infer_fields_measure_psf", 32)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header, re.S)
        assert m, f"{name} is not declared in include/debvader_hip.h"
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)         # bound: the library exports it
        restype, argtypes = _lib.SIGNATURES[name]
        want = [ctype[t] for t in _c_types(m.group(1))]
        assert restype is C.c_int and len(argtypes) == len(want) == nargs
        for i, (a, w) in enumerate(zip(argtypes, want)):
            assert a is w, (name, i, a, w)
        assert getattr(_lib.lib, name).argtypes == argtypes
    assert _lib.SIGNATURES["dv_infer_fields_measure_psf"][1][:20] == _lib.SIGNATURES["dv_infer_fields_measure"][1]
    src = open(os.path.join(ROOT, "debvader_amd", "csrc", "Makefile")).read()
    assert "regauss.hip" in src and os.path.exists(os.path.join(ROOT, "debvader_amd", "csrc", "regauss.hip"))
    # no existing entry point changed its signature and no environment variable was added
    assert "getenv" not in open(os.path.join(ROOT, "debvader_amd", "csrc", "regauss.hip")).read()
