"""CPU checks of the catalogue measurement: the numpy restatement of the algorithm on inputs whose
answer is known, and the Python layer - debvader_amd.measure.measurement and DeblendFieldBatch.deblend_fields(measure=True)
- over the stand-in engine of tests/stub_measure_engine.py.  No GPU is touched."""
import inspect

import numpy as np
import pytest

from tests import measure_oracle as mo
from tests.stub_measure_engine import CS, NB, Net, OracleContext, stub_catalogue

GAUSSIANS = [(59, (6.0, 2.0, 11.0), (1.3, -2.1)), (59, (4.0, -1.5, 5.0), (-3.2, 0.7)), (59, (16.0, 5.0, 9.0), (2.5, 2.5)),
             (31, (2.25, 0.0, 2.25), (0.5, 0.5))]


@pytest.mark.parametrize("cs,M,offset", GAUSSIANS)
def test_oracle_recovers_noise_free_elliptical_gaussians(cs, M, offset):
    """Gaussians whose 3.5 sigma extent fits the stamp: the matched Gaussian is the iteration's fixed point"""
    shape, iters, status = mo.adaptive_moments(mo.gaussian_stamp(cs, M, offset))
    ctr = (cs - 1) / 2.0
    dc = max(abs(shape[0] - ctr - offset[0]), abs(shape[1] - ctr - offset[1]))
    dm = np.abs(shape[2:] - np.array(M)).max()
    print(f"cs {cs} M {M} offset {offset}: status {status}, {iters} iterations, centre off by {dc:.2e} px, M by {dm:.2e}")
    assert status == mo.CONVERGED
    assert dc <= 1e-6
    assert dm <= 1e-5
    assert iters <= 60


def test_oracle_degenerate_stamps_and_iteration_limit():
    for cs in (31, 59):
        shape, iters, status = mo.adaptive_moments(np.zeros((cs, cs)))
        assert (status, iters) == (mo.FAILED, 1)                       # S0 = 0 at the first iteration
        assert shape.tolist() == [(cs - 1) / 2.0, (cs - 1) / 2.0, 9.0, 0.0, 9.0]
        spike = np.zeros((cs, cs))
        spike[cs // 2, cs // 2] = 7.0
        shape, iters, status = mo.adaptive_moments(spike)
        assert (status, iters) == (mo.FAILED, 2)                       # M = 0 after the first: det = 0 exactly
        assert shape.tolist() == [(cs - 1) / 2.0, (cs - 1) / 2.0, 0.0, 0.0, 0.0]
    g = mo.gaussian_stamp(31, (6.0, 2.0, 11.0), (1.3, -2.1))
    shape, iters, status = mo.adaptive_moments(g, sigma0=2.5, max_iter=0)
    assert (status, iters) == (mo.ITER_LIMIT, 0) and shape.tolist() == [15.0, 15.0, 6.25, 0.0, 6.25]
    shape, iters, status = mo.adaptive_moments(g, max_iter=5)
    assert (status, iters) == (mo.ITER_LIMIT, 5)


def test_oracle_fluxes():
    rng = np.random.default_rng(2)
    P = rng.uniform(size=(3, 9, 9, 4)).astype(np.float32)
    S = rng.uniform(size=(3, 9, 9, 4)).astype(np.float32)
    out = mo.measure(P, S, band=1)
    assert np.allclose(out["flux"], P.astype(np.float64).sum(axis=(1, 2)), rtol=1e-14)
    assert np.allclose(out["flux_err"], np.sqrt((S.astype(np.float64) ** 2).sum(axis=(1, 2))), rtol=1e-14)
    assert mo.measure(P, None, band=1)["flux_err"] is None


def test_measure_stamps_columns_and_derived_values():
    from debvader_amd.measure.measurement import catalogue_dtype, measure_stamps

    ctx = OracleContext()
    stamps = [mo.gaussian_stamp(31, (6.0, 2.0, 11.0), (1.3, -2.1)), mo.gaussian_stamp(31, (2.25, 0.0, 2.25), (0.5, 0.5)),
              np.zeros((31, 31))]
    mean = np.stack(stamps)[:, :, :, None] * np.array([1.0, 2.0, 3.0])
    std = np.full(mean.shape, 0.5)
    rec = measure_stamps(mean, std, ctx=ctx)
    assert isinstance(rec, np.recarray) and rec.dtype == np.dtype(catalogue_dtype(3))
    assert rec.dtype.names == ("flux", "flux_err", "row", "col", "Mrr", "Mrc", "Mcc", "iters", "status", "sigma", "e1", "e2")
    assert rec["flux"].shape == (3, 3) and rec["flux_err"].shape == (3, 3)
    assert rec["flux"].dtype == np.float64 and rec["iters"].dtype == np.int32 and rec["status"].dtype == np.int32
    assert ctx.calls == [dict(n=3, band=2, sigma0=3.0, tol=1e-10, max_iter=200, dtype=np.float32, with_stddev=True)]
    assert rec["status"].tolist() == [0, 0, 3]
    assert np.allclose(rec["flux_err"], 0.5 * 31)
    assert np.allclose(rec["flux"][:, 1], 2 * rec["flux"][:, 0])
    # the formulas, on the values of the recarray itself
    ok = rec["status"] == 0
    det = rec["Mrr"] * rec["Mcc"] - rec["Mrc"] ** 2
    assert np.array_equal(rec["sigma"][ok], np.sqrt(np.sqrt(det[ok])))
    assert np.array_equal(rec["e1"][ok], ((rec["Mcc"] - rec["Mrr"]) / (rec["Mcc"] + rec["Mrr"]))[ok])
    assert np.array_equal(rec["e2"][ok], (2.0 * rec["Mrc"] / (rec["Mcc"] + rec["Mrr"]))[ok])
    assert abs(rec["sigma"][0] - (6.0 * 11.0 - 4.0) ** 0.25) < 1e-5 and abs(rec["e1"][0] - 5.0 / 17.0) < 1e-5
    assert abs(rec["e2"][0] - 4.0 / 17.0) < 1e-5 and abs(rec["e1"][1]) < 1e-6
    # NaN where the measurement failed; what the kernel left is still there
    assert np.isnan(rec["sigma"][2]) and np.isnan(rec["e1"][2]) and np.isnan(rec["e2"][2])
    assert rec["Mrr"][2] == 9.0 and rec["row"][2] == 15.0
    # without stddev stamps, and with other parameters
    rec = measure_stamps(mean, band=0, sigma0=2.0, tol=1e-8, max_iter=0, ctx=ctx)
    assert ctx.calls[-1] == dict(n=3, band=0, sigma0=2.0, tol=1e-8, max_iter=0, dtype=np.float32, with_stddev=False)
    assert np.isnan(rec["flux_err"]).all() and (rec["status"] == 2).all() and (rec["Mrr"] == 4.0).all()
    assert measure_stamps(np.zeros((0, 31, 31, 3)), ctx=ctx).shape == (0,)


def test_measure_stamps_argument_checks():
    from debvader_amd import engine as E
    from debvader_amd.measure.measurement import measure_stamps

    sig = inspect.signature(measure_stamps).parameters
    assert list(sig) == ["mean", "stddev", "band", "sigma0", "tol", "max_iter", "ctx"]
    assert [sig[k].default for k in list(sig)[1:]] == [None, 2, 3.0, 1e-10, 200, None]
    ctx, good = OracleContext(), np.zeros((2, 31, 31, 3))
    for kw, msg in [(dict(band=3), "band"), (dict(band=-1), "band"), (dict(band=1.5), "band"), (dict(sigma0=0.0), "sigma0"),
                    (dict(sigma0=np.nan), "sigma0"), (dict(tol=-1e-3), "tol"), (dict(tol=np.inf), "tol"),
                    (dict(max_iter=-1), "max_iter")]:
        with pytest.raises(ValueError, match=msg):
            measure_stamps(good, ctx=ctx, **kw)
    with pytest.raises(ValueError, match="square stamps"):
        measure_stamps(np.zeros((2, 31, 30, 3)), ctx=ctx)
    with pytest.raises(ValueError, match="square stamps"):
        measure_stamps(np.zeros((31, 31, 3)), ctx=ctx)
    with pytest.raises(ValueError, match="stddev stamps"):
        measure_stamps(good, np.zeros((2, 31, 31, 2)), ctx=ctx)
    with pytest.raises(ValueError, match="at most 90"):
        measure_stamps(np.zeros((1, 91, 91, 1)), band=0, ctx=ctx)
    assert ctx.calls == []
    # the unbound engine methods validate before they touch a handle: a bare object stands in
    with pytest.raises(ValueError, match="band"):
        E.Context.scene_measure(object(), good, band=5)
    with pytest.raises(ValueError, match="places"):
        E.Engine.infer_fields_measure(object(), np.zeros((1, 81, 81, 6)), [[0, 0]], [0, 1])
    with pytest.raises(ValueError, match="max_iter"):
        E.Engine.infer_fields_measure(object(), np.zeros((1, 81, 81, 6)), [[0, 0]], [0, 1], places=[[0, 0]], max_iter=-2)
    with pytest.raises(ValueError, match="field_ptr"):
        E.Engine.infer_fields_measure(object(), np.zeros((1, 81, 81, 6)), [[0, 0]], [0, 2], return_fields=False)


def test_abi_struct_and_signatures():
    from debvader_amd import _lib

    par = _lib.DvMeasureParams()
    assert _lib.lib.dv_measure_params_default(par) == 0
    assert (par.band, par.sigma0, par.tol, par.max_iter) == (2, 3.0, 1e-10, 200)
    assert _lib.lib.dv_measure_params_default(None) == -1
    for name in ("dv_measure_params_default", "dv_scene_measure", "dv_infer_fields_measure"):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["dv_scene_measure"][1]) == 12 and len(_lib.SIGNATURES["dv_infer_fields_measure"][1]) == 20


F = 81
DIST = [np.array([[0.0, 0.0], [5.0, -7.0]]), np.zeros((0, 2)), np.array([[100.0, 0.0], [-3.0, 11.0]]), np.array([[0.0, 40.0]])]


def _batch():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch

    net = Net()
    return net, DeblendFieldBatch(net, np.random.default_rng(3).normal(size=(4, F, F, NB)), CS, NB)


def test_deblend_fields_defaults_are_unchanged():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch

    sig = inspect.signature(DeblendFieldBatch.deblend_fields).parameters
    assert sig["measure"].default is False and sig["return_fields"].default is True
    net, b = _batch()
    res = b.deblend_fields(DIST, on_device=True)
    assert [c[0] for c in net._core.engine.calls] == ["set_normalise", "infer_fields_composite", "set_normalise"]
    for rec in res:
        assert rec.dtype == np.dtype(DeblendFieldBatch.ON_DEVICE_COLUMNS)
    res = b.deblend_fields(DIST)
    for rec in res:
        assert rec.dtype == np.dtype(DeblendFieldBatch.DEFAULT_COLUMNS)
    assert net._core.ctx.calls == []


def test_deblend_fields_measure_on_device():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch

    net, b = _batch()
    res = b.deblend_fields(DIST, on_device=True, measure=True)
    call = [c for c in net._core.engine.calls if c[0] == "infer_fields_measure"]
    assert len(call) == 1 and call[0][1] == 8 and call[0][2] is True
    assert np.array_equal(call[0][3], int((F - CS) / 2) + np.array([[0, 0], [5, -7], [-3, 11]]))
    want = np.dtype(DeblendFieldBatch.ON_DEVICE_COLUMNS + DeblendFieldBatch.measure_columns(NB))
    cat = stub_catalogue(3)
    assert [len(r) for r in res] == [2, 0, 1, 0]
    rows = [(0, 0), (0, 1), (2, 0)]                       # (field, row) of global stamps 0, 1, 2
    starts = -29 + np.array([[0, 0], [5, -7], [-3, 11]]) + 40
    for i, (m, k) in enumerate(rows):
        rec = res[m]
        assert rec.dtype == want
        assert np.array_equal(rec["flux"][k], cat["flux"][i]) and np.array_equal(rec["flux_err"][k], cat["flux_err"][i])
        assert [rec[n][k] for n in ("row", "col", "Mrr", "Mrc", "Mcc")] == cat["shape"][i].tolist()
        assert rec["iters"][k] == cat["iters"][i] and rec["status"][k] == cat["status"][i]
        assert rec["measured_distance_x"][k] == starts[i, 0] + cat["shape"][i, 0] - 40
        assert rec["measured_distance_y"][k] == starts[i, 1] + cat["shape"][i, 1] - 40
        assert rec["mse_center"][k] == 60.0 * i
    assert np.isnan(res[2]["sigma"][0]) and res[0]["sigma"][0] == (4.0 * 9.0 - 0.25) ** 0.25
    assert res[1].dtype == want
    assert b.get_predicted_fields()["predicted_mean_fields"].shape == (4, F, F, NB)
    # the catalogue-only call: no placements go down, no fields come back
    res2 = b.deblend_fields(DIST, on_device=True, measure=True, return_fields=False)
    call = [c for c in net._core.engine.calls if c[0] == "infer_fields_measure"][-1]
    assert call[2] is False and call[3] is None
    for r, r2 in zip(res, res2):
        assert r2.dtype == want
        for n in ("flux", "row", "Mcc", "status", "measured_distance_x", "mse_center", "passed_cuts"):
            assert np.array_equal(r[n], r2[n]), n
    with pytest.raises(ValueError, match="catalogue-only"):
        b.get_predicted_fields()
    with pytest.raises(ValueError, match="catalogue-only"):
        b.get_residual_fields()


def test_deblend_fields_measure_on_the_default_path_uses_measure_stamps():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch

    net, b = _batch()
    res = b.deblend_fields(DIST, measure=True)
    assert [c["n"] for c in net._core.ctx.calls] == [3] and net._core.ctx.calls[0]["with_stddev"]
    want = np.dtype(DeblendFieldBatch.DEFAULT_COLUMNS + DeblendFieldBatch.measure_columns(NB))
    assert all(r.dtype == want for r in res)
    # stamp i holds a round blob at offset (0.5 i, -0.25 i) from the stamp centre: stamp 1 is row 1 of field 0
    rec = res[0]
    assert rec["status"].tolist() == [0, 0]
    assert abs(rec["row"][1] - 29.5) < 1e-6 and abs(rec["col"][1] - 28.75) < 1e-6 and abs(rec["Mrr"][1] - 5.0) < 1e-4
    assert abs(rec["measured_distance_x"][1] - 5.5) < 1e-6 and abs(rec["measured_distance_y"][1] - (-7.25)) < 1e-6
    assert abs(res[2]["measured_distance_x"][0] - (-3.0 + 1.0)) < 1e-6
    assert np.allclose(rec["flux_err"], 0.5 * CS)


def test_deblend_fields_refuses_unsupported_combinations():
    net, b = _batch()
    with pytest.raises(ValueError, match="position-fit or Monte-Carlo"):
        b.deblend_fields(DIST, on_device=True, measure=True, optimise_positions=True)
    with pytest.raises(ValueError, match="position-fit or Monte-Carlo"):
        b.deblend_fields(DIST, measure=True, epistemic_uncertainty_estimation=True)
    with pytest.raises(ValueError, match="catalogue-only"):
        b.deblend_fields(DIST, on_device=True, return_fields=False)
    with pytest.raises(ValueError, match="catalogue-only"):
        b.deblend_fields(DIST, measure=True, return_fields=False)
    assert net._core.engine.calls == []
