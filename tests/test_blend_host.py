"""CPU checks of the blendedness column: the numpy restatement of the definition on inputs whose
answer is known, the Python layer - debvader_amd.measure.measurement.measure_blendedness and
DeblendFieldBatch.deblend_fields(blendedness=True) - over the stand-in engine of tests/stub_blend_engine.py, and the ABI.  No
GPU is touched."""
import inspect
import os
import re

import numpy as np
import pytest

from tests import blend_oracle as bo
from tests import measure_oracle as mo
from tests.stub_blend_engine import CS, NB, Net, OracleContext, stub_blend
from tests.stub_measure_engine import stub_catalogue

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gauss_row(cs, s2, off=(0.0, 0.0)):
    ctr = (cs - 1) / 2.0
    return [ctr + off[0], ctr + off[1], s2, 0.0, s2]


def test_oracle_lone_gaussian_has_blendedness_zero():
    cs, F = 31, 64
    P = mo.gaussian_stamp(cs, (4.0, 1.0, 6.0), (0.7, -1.1))[None, :, :, None].astype(np.float32) * np.ones(3, np.float32)
    shape, status = [[15.7, 13.9, 4.0, 1.0, 6.0]], [0]
    for place in ([10, 20], [-9, 50], [-40, 3]):                     # inside, over a corner, wholly outside
        T = bo.composite(P, [place], [0, 1], 1, F)
        out = bo.blend(P, shape, status, [place], T, T + 0.25)
        W, A, Bm, Bd = out["blend"][0]
        assert A == Bm                                                # T holds the widened stamp values, nothing else
        if place[0] <= -cs:
            assert out["npix"][0] == 0 and out["blend"][0].tolist() == [0.0] * 4
            assert all(np.isnan(r[0]) for r in bo.ratios(out["blend"], out["npix"]))
        else:
            assert bo.ratios(out["blend"], out["npix"])[0][0] == 0.0
            assert Bd == pytest.approx(A + 0.25 * W, rel=1e-12) and W > 0 and A > 0


def test_oracle_two_equal_gaussians_closed_form_and_monotony():
    """Matched weights: A = pi s^2, the neighbour adds pi s^2 exp(-d^2 / (4 s^2)): blendedness = e / (1 + e)"""
    cs, F, s2 = 59, 120, 9.0
    g = mo.gaussian_stamp(cs, (s2, 0.0, s2), (0.0, 0.0))
    P = np.stack([g, g])[:, :, :, None].astype(np.float32) * np.ones(3, np.float32)
    shape, status = [_gauss_row(cs, s2)] * 2, [0, 0]
    last = 1.0
    for d in (2, 4, 7, 11, 16):
        places = [[30, 30], [30, 30 + d]]
        T = bo.composite(P, places, [0, 2], 1, F)
        out = bo.blend(P, shape, status, places, T)
        b = bo.ratios(out["blend"], out["npix"])[0]
        e = np.exp(-d * d / (4.0 * s2))
        print(f"d = {d:2d}: blendedness {b[0]:.9f}, closed form {e / (1 + e):.9f}")
        assert abs(b[0] - e / (1 + e)) < 1e-6 and b[0] == pytest.approx(b[1], abs=1e-12)
        assert b[0] < last                                            # rises as the neighbour approaches
        last = b[0]
        assert out["blend"][0, 1] == pytest.approx(np.pi * s2, rel=1e-6)
        assert np.isnan(out["blend"][:, 3]).all()                     # no data field
    assert last < 1e-3


def test_oracle_clipping_and_ineligible_rows():
    cs, F = 31, 64
    rng = np.random.default_rng(5)
    P = rng.uniform(0.1, 1.0, size=(6, cs, cs, 3)).astype(np.float32)
    places = [[-10, -4], [50, 40], [5, 5], [5, 5], [5, 5], [5, 5]]
    row = [14.2, 15.9, 5.0, -1.0, 7.0]
    shape = [row, row, row, [14.2, np.nan, 5.0, 0.0, 7.0], [15.0, 15.0, 1e-3, 0.0, 1e-3], row]
    status = [0, 2, 3, 0, 0, 1]
    T = bo.composite(P, places, [0, 6], 1, F)
    D = rng.normal(size=T.shape)
    out = bo.blend(P, shape, status, places, T, D)
    assert out["npix"].tolist() == [21 * 27, 14 * 24, -1, -1, -1, -1]
    assert np.isnan(out["blend"][2:]).all() and np.isfinite(out["blend"][:2]).all()
    # the clipped sums, by hand
    g = bo.weights(cs, row)
    assert out["blend"][0, 0] == pytest.approx(g[10:, 4:].sum(), rel=1e-13)
    assert out["blend"][0, 3] == pytest.approx((g[10:, 4:] * D[0, :21, :27, 2]).sum(), rel=1e-12, abs=1e-12)
    assert out["blend"][1, 1] == pytest.approx((g[:14, :24] * P[1, :14, :24, 2].astype(np.float64)).sum(), rel=1e-13)
    bl, bld = bo.ratios(out["blend"], out["npix"])
    assert np.isnan(bl[2:]).all() and np.isnan(bld[2:]).all() and np.isfinite(bl[:2]).all()


def test_oracle_raster_order_against_pairwise_stays_inside_the_bound():
    """The bound of the GPU test, 1e-12 sum g |x|, holds between two summation orders of the restatement itself"""
    cs, F = 59, 97
    rng = np.random.default_rng(9)
    P = rng.normal(0.3, 1.0, size=(8, cs, cs, 6)).astype(np.float32)
    places = rng.integers(-20, F - 30, size=(8, 2))
    shape = [[29.0 + rng.normal(), 29.0 + rng.normal(), 8.0, 2.0, 11.0] for _ in range(8)]
    T = bo.composite(P, places, [0, 8], 1, F)
    D = T + rng.normal(size=T.shape)
    a = bo.blend(P, shape, [0] * 8, places, T, D)
    b = bo.blend(P, shape, [0] * 8, places, T, D, total=lambda x: float(np.sum(x)))
    d = np.abs(a["blend"][:, 1:] - b["blend"][:, 1:]) / a["abs"]
    print(f"raster against pairwise: at most {d.max():.2e} of sum g |x|")
    assert np.array_equal(a["npix"], b["npix"]) and d.max() <= 1e-12
    assert (np.abs(a["blend"][:, 0] - b["blend"][:, 0]) <= 1e-12 * a["blend"][:, 0]).all()


def test_measure_blendedness_columns_and_nan_rules():
    from debvader_amd.measure.measurement import blend_dtype, blend_records, measure_blendedness, measure_stamps

    names = ("blend_weight", "blend_child", "blend_model", "blend_data", "blend_npix", "blendedness", "blendedness_data")
    assert tuple(n for n, _ in blend_dtype()) == names
    st = stub_blend(6)
    rec = blend_records(st["blend"], st["npix"])
    assert rec.dtype == np.dtype(blend_dtype()) and rec.dtype.names == names
    assert rec["blend_npix"].dtype == np.int32 and rec["blend_npix"].tolist() == st["npix"].tolist()
    assert np.array_equal(rec["blend_child"], st["blend"][:, 1], equal_nan=True)
    assert rec["blendedness"][0] == 1.0 - 2.0 / 4.0 and rec["blendedness_data"][0] == 1.0 - 2.0 / 8.0
    assert np.isnan(rec["blendedness"][1]) and rec["blendedness_data"][1] == 1.0 - 3.0 / 9.0          # Bm = 0
    assert np.isnan(rec["blendedness"][2]) and np.isnan(rec["blendedness_data"][2])                   # ineligible
    assert rec["blendedness"][3] == 1.0 - 5.0 / 10.0 and np.isnan(rec["blendedness_data"][3])         # Bd < 0
    assert np.isnan(rec["blendedness"][4]) and np.isnan(rec["blendedness_data"][4])                   # wholly outside
    assert rec["blendedness"][5] == 1.0 - 7.0 / 14.0
    # through the context: two overlapping blobs and a failed one, in one field given without its leading axis
    ctx = OracleContext()
    blobs = [mo.gaussian_stamp(31, (4.0, 0.0, 4.0), (0.0, 0.0)), mo.gaussian_stamp(31, (4.0, 0.0, 4.0), (1.0, 0.0)),
             np.zeros((31, 31))]
    mean = (np.stack(blobs)[:, :, :, None] * np.ones(3)).astype(np.float32)
    cat = measure_stamps(mean, ctx=ctx)
    places = [[10, 10], [10, 14], [30, 30]]
    T = bo.composite(mean, places, [0, 3], 1, 80)[0]
    got = measure_blendedness(mean, cat, places, T, ctx=ctx)
    assert got.dtype == np.dtype(blend_dtype()) and ctx.calls[-1] == dict(n=3, band=2, with_data=False, field_ptr=None,
                                                                            fields=(1, 80, 80, 3))
    assert got["blend_npix"].tolist() == [961, 961, -1] and np.isnan(got["blend_data"]).all()
    assert np.isnan(got["blendedness"][2]) and np.isnan(got["blendedness_data"]).all()
    e = np.exp(-17.0 / 16.0)                                           # the centroids are (1, 4) px apart, s^2 = 4
    assert abs(got["blendedness"][0] - e / (1 + e)) < 1e-5 and abs(got["blendedness"][1] - e / (1 + e)) < 1e-5
    both = measure_blendedness(mean, cat, places, T[None], T[None] * 2.0, field_ptr=[0, 3], ctx=ctx)
    assert ctx.calls[-1]["with_data"] and ctx.calls[-1]["field_ptr"] == [0, 3]
    assert np.allclose(both["blendedness_data"][:2], 1.0 - 0.5 * (1.0 - got["blendedness"][:2]), rtol=1e-12)
    sig = inspect.signature(measure_blendedness).parameters
    assert list(sig)[:6] == ["stamps_mean", "catalogue", "places", "model_fields", "data_fields", "field_ptr"]
    assert sig["data_fields"].default is None and sig["field_ptr"].default is None


def test_engine_methods_check_before_they_touch_a_handle():
    from debvader_amd import engine as E

    good = np.zeros((2, 31, 31, 3), np.float32)
    sh, st, pl, T = np.zeros((2, 5)), np.zeros(2, np.int32), np.zeros((2, 2), np.int32), np.zeros((1, 40, 40, 3))
    for args, msg in [((np.zeros((2, 31, 30, 3)), sh, st, pl, T), "square stamps"), ((good, sh, st, pl, T[..., :2]), "model fields"),
                      ((good, sh[:1], st, pl, T), "expected shape"), ((good, sh, st, pl, np.zeros((2, 40, 40, 3))), "field_ptr")]:
        with pytest.raises(ValueError, match=msg):
            E.Context.scene_blend(object(), *args)
    with pytest.raises(ValueError, match="data fields"):
        E.Context.scene_blend(object(), good, sh, st, pl, T, np.zeros((1, 41, 41, 3)))
    with pytest.raises(ValueError, match="band"):
        E.Context.scene_blend(object(), good, sh, st, pl, T, band=3)
    with pytest.raises(ValueError, match="places"):
        E.Engine.infer_fields_measure_blend(object(), np.zeros((1, 81, 81, 6)), [[0, 0]], [0, 1], None, return_fields=False)
    with pytest.raises(ValueError, match="max_iter"):
        E.Engine.infer_fields_measure_blend(object(), np.zeros((1, 81, 81, 6)), [[0, 0]], [0, 1], [[0, 0]], max_iter=-2)
    for name in ("scene_blend", "infer_fields_measure_blend", "infer_cutouts_measure_blend"):
        assert callable(getattr(E.Engine, name))


def test_abi_declared_exported_and_bound():
    from debvader_amd import _lib

    header = open(os.path.join(ROOT, "include", "debvader_hip.h")).read()
    exports = open(os.path.join(ROOT, "debvader_amd", "csrc", "exports.map")).read()
    assert "dv_*" in exports
    for name, nargs in (("dv_scene_blend", 16), ("dv_infer_fields_measure_blend", 22)):
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert decl is not None and len(decl.group(1).split(",")) == nargs, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name][1]         # the loaded library exports it
    # the blendedness call takes dv_infer_fields_measure's arguments, then its own two
    assert _lib.SIGNATURES["dv_infer_fields_measure_blend"][1][:20] == _lib.SIGNATURES["dv_infer_fields_measure"][1]


F = 81
DIST = [np.array([[0.0, 0.0], [5.0, -7.0]]), np.zeros((0, 2)), np.array([[100.0, 0.0], [-3.0, 11.0]]), np.array([[0.0, 40.0]])]


def _batch():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch

    net = Net()
    return net, DeblendFieldBatch(net, np.random.default_rng(3).normal(size=(4, F, F, NB)), CS, NB)


def test_deblend_fields_blendedness_columns():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch
    from debvader_amd.measure.measurement import blend_dtype, blend_records

    assert inspect.signature(DeblendFieldBatch.deblend_fields).parameters["blendedness"].default is False
    assert DeblendFieldBatch.blend_columns() == blend_dtype()
    net, b = _batch()
    res = b.deblend_fields(DIST, on_device=True, measure=True, blendedness=True)
    calls = [c for c in net._core.engine.calls if c[0].startswith("infer_fields")]
    assert [c[0] for c in calls] == ["infer_fields_measure_blend"] and calls[0][1] == 8 and calls[0][2] is True
    assert np.array_equal(calls[0][3], int((F - CS) / 2) + np.array([[0, 0], [5, -7], [-3, 11]]))
    want = np.dtype(DeblendFieldBatch.ON_DEVICE_COLUMNS + DeblendFieldBatch.measure_columns(NB) + blend_dtype())
    ref = blend_records(**stub_blend(3))
    cat = stub_catalogue(3)
    assert [len(r) for r in res] == [2, 0, 1, 0] and all(r.dtype == want for r in res)
    for i, (m, k) in enumerate([(0, 0), (0, 1), (2, 0)]):
        for name in ref.dtype.names:
            assert np.array_equal(res[m][name][k], ref[name][i], equal_nan=True), (i, name)
        assert np.array_equal(res[m]["flux"][k], cat["flux"][i]) and res[m]["mse_center"][k] == 60.0 * i
    assert np.isnan(res[0]["blendedness"][1]) and res[0]["blendedness"][0] == 0.5 and np.isnan(res[2]["blendedness"][0])
    assert b.get_predicted_fields()["predicted_mean_fields"].shape == (4, F, F, NB)
    # without the fields: the placements still go down, the same columns come back
    res2 = b.deblend_fields(DIST, on_device=True, measure=True, blendedness=True, return_fields=False)
    call = [c for c in net._core.engine.calls if c[0] == "infer_fields_measure_blend"][-1]
    assert call[2] is False and np.array_equal(call[3], calls[0][3])
    for r, r2 in zip(res, res2):
        assert r2.dtype == want
        for name in ("flux", "status", "mse_center", "passed_cuts") + ref.dtype.names:
            assert np.array_equal(r[name], r2[name], equal_nan=r.dtype[name].kind == "f"), name
    with pytest.raises(ValueError, match="catalogue-only"):
        b.get_predicted_fields()
    # the call without the keyword is where it was
    net, b = _batch()
    plain = b.deblend_fields(DIST, on_device=True, measure=True)
    assert [c[0] for c in net._core.engine.calls if c[0].startswith("infer_fields")] == ["infer_fields_measure"]
    assert all(r.dtype == np.dtype(DeblendFieldBatch.ON_DEVICE_COLUMNS + DeblendFieldBatch.measure_columns(NB)) for r in plain)


def test_deblend_fields_refuses_unsupported_blendedness_combinations():
    net, b = _batch()
    for kw, msg in [(dict(on_device=True), "needs measure=True"), (dict(), "needs measure=True"),
                    (dict(measure=True), "needs on_device=True"),
                    (dict(on_device=True, measure=True, optimise_positions=True), "cannot be combined"),
                    (dict(on_device=True, measure=True, epistemic_uncertainty_estimation=True), "cannot be combined"),
                    (dict(on_device=True, measure=True, measure_samples=4), "cannot be combined"),
                    (dict(on_device=True, measure=True, measure_samples=4, return_fields=False), "cannot be combined")]:
        with pytest.raises(ValueError, match="blendedness=True " + msg):
            b.deblend_fields(DIST, blendedness=True, **kw)
    assert net._core.engine.calls == []
