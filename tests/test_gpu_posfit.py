"""The batched sub-pixel position fit (dv_scene_fit_shifts, deblend_cutout/optimization.py, DeblendField.optimise_positions)
against a scipy restatement of the reference's objective, the reference's own results (tests/golden/posfit.npz), known
truth and the compositing that consumes the fitted shifts."""
import os

import numpy as np
import pytest
import scipy.ndimage

from oracle import scene_oracle as so

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _ctx():
    from debvader_amd import engine as E
    return E.default_context()


def _pad(stamp_r, F):
    cs = stamp_r.shape[0]
    po = int((F - cs) / 2)
    out = np.zeros((F, F))
    out[po:po + cs, po:po + cs] = stamp_r
    return out


def _objective(field_r, stamp_r, d, s):
    """the reference's J (optimization.py): mean((img - shift(shift(pad(stamp), d), s))^2) over the whole field"""
    net = scipy.ndimage.shift(_pad(stamp_r, field_r.shape[0]), shift=(d[0], d[1]))
    return np.square(field_r - scipy.ndimage.shift(net, shift=(s[0], s[1]))).mean()


def _gauss(cs, sig, amp, e=0.0, c=(0.0, 0.0)):
    y, x = np.mgrid[:cs, :cs] - (cs - 1) / 2.0
    return amp * np.exp(-0.5 * (((x - c[1]) / sig) ** 2 + ((y - c[0]) / (sig * (1 + e))) ** 2))


def _bands(a, nb):
    out = np.zeros(a.shape + (nb,))
    out[..., 2] = a
    out[..., 0] = 0.5 * a          # other bands must not matter
    return out


def test_objective_matches_scipy_restatement():
    from debvader_amd.deblend_cutout.optimization import position_optimization_batch

    rng = np.random.default_rng(1)
    F, cs = 97, 31
    field = rng.normal(0, 0.3, size=(F, F))
    stamps = np.array([_gauss(cs, 3.0, 5.0, 0.2), _gauss(cs, 2.0, 3.0, -0.3, (1.0, -2.0)), rng.random((cs, cs)),
                       _gauss(cs, 4.0, 2.0), rng.random((cs, cs))])
    # integer, fractional, near the edge (within 20 px), the stamp partly outside the field, fractional near the edge
    dist = np.array([[0.0, 0.0], [2.4, -3.7], [-30.0, 28.0], [40.0, -5.0], [-31.5, 29.25]])
    starts = np.array([[0.7, -1.3], [-2.2, 0.4], [1.9, 2.6], [-0.3, -4.5], [2.5, -1.75]])
    for nb in (3, 6):
        got = _ctx().scene_fit_shifts(field, stamps, dist, shifts=starts, max_iter=0)
        np.testing.assert_array_equal(got["shifts"], starts)
        assert (got["status"] == 2).all() and (got["iters"] == 0).all()
        exp = np.array([_objective(field, st, d, s0) for st, d, s0 in zip(stamps, dist, starts)])
        np.testing.assert_allclose(got["objective"], exp, rtol=1e-10, atol=0)
        # the same through the public batch form with 3 and 6 bands (r band = index 2)
        _, det = position_optimization_batch(_bands(field, nb), _bands(stamps, nb), dist, max_iter=0, return_details=True)
        np.testing.assert_allclose(det["objective"], [_objective(field, st, d, (0, 0)) for st, d in zip(stamps, dist)],
                                   rtol=1e-10, atol=0)
    # the cs = F single-galaxy form: a padded image, integer and fractional distances
    padded = _pad(stamps[0], F)
    for d in ([3.0, -2.0], [1.5, -0.25]):
        got = _ctx().scene_fit_shifts(field, padded[None], [d], shifts=[[0.4, -0.9]], max_iter=0)
        np.testing.assert_allclose(got["objective"][0], _objective(field, padded, d, (0.4, -0.9)), rtol=1e-10, atol=0)


def test_large_shifts_and_bounds_read_nothing_outside_the_field():
    """A shift beyond the field (|s| > F - 1) maps no pixel into it: shift(net, s) = 0 and J = mean(field^2).  The reach
    the workspace is sized for is capped at F, so such starts and bounds cost a field-sized window, not one sized by the
    shift; inputs beyond the documented +-1e6 are refused."""
    from debvader_amd._lib import DvError

    rng = np.random.default_rng(11)
    F, cs = 97, 31
    field = rng.normal(0, 0.3, size=(F, F))
    stamps = np.array([_gauss(cs, 3.0, 5.0, 0.2), rng.random((cs, cs)), _gauss(cs, 2.0, 3.0), rng.random((cs, cs)),
                       _gauss(cs, 2.5, 4.0)])
    dist = np.array([[0.0, 0.0], [2.5, -1.25], [10.0, -20.0], [-3.0, 4.0], [1.0, 1.0]])
    starts = np.array([[3.0e4, 0.0], [-5.0e5, 2.0], [0.5, 9.0e5], [100.0, -100.0], [40.0, -30.0]])
    ctx = _ctx()
    got = ctx.scene_fit_shifts(field, stamps, dist, shifts=starts, max_iter=0)
    np.testing.assert_array_equal(got["shifts"], starts)
    np.testing.assert_allclose(got["objective"][:4], np.mean(field ** 2), rtol=1e-12, atol=0)
    np.testing.assert_allclose(got["objective"][4], _objective(field, stamps[4], dist[4], starts[4]), rtol=1e-10, atol=0)
    # a box far wider than the field: the fit stays finite and ends where J is no higher than at the start
    r = ctx.scene_fit_shifts(field, stamps, dist, bound=1.0e5)
    j0 = ctx.scene_fit_shifts(field, stamps, dist, max_iter=0)["objective"]
    assert np.isfinite(r["shifts"]).all() and (r["objective"] <= j0).all() and (r["status"] != 2).all(), r
    for bad in (dict(shifts=[[2.0e6, 0.0]] * 5, max_iter=0), dict(bound=2.0e6)):
        with pytest.raises(DvError):
            ctx.scene_fit_shifts(field, stamps, dist, **bad)


def test_fewer_than_three_bands_raises():
    from debvader_amd.deblend_cutout.optimization import position_optimization, position_optimization_batch

    F, cs = 41, 11
    with pytest.raises(ValueError, match="band"):
        position_optimization_batch(np.zeros((F, F, 2)), np.zeros((1, cs, cs, 2)), [[0, 0]])
    with pytest.raises(ValueError, match="band"):
        position_optimization(np.zeros((F, F, 2)), np.zeros((F, F, 2)), [0, 0])


def test_against_the_reference_fixture():
    z = np.load(os.path.join(HERE, "golden", "posfit.npz"))
    for kind in ("real", "syn"):
        field, stamps, dist = z[f"{kind}_field_r"], z[f"{kind}_stamps_r"], z[f"{kind}_dist"]
        r = _ctx().scene_fit_shifts(field, stamps, dist, bound=3.0)
        ref_s, ref_j = z[f"{kind}_shift"], z[f"{kind}_objective"]
        assert (r["objective"] <= ref_j * (1 + 1e-9)).all(), (kind, r["objective"], ref_j)
        np.testing.assert_allclose(r["shifts"], ref_s, rtol=0, atol=5e-3, err_msg=kind)
        assert (r["status"] != 2).all(), r
        # the engine's J at its shifts is the reference's formula there
        exp = np.array([_objective(field, st, d, s) for st, d, s in zip(stamps, dist, r["shifts"])])
        np.testing.assert_allclose(r["objective"], exp, rtol=1e-10, atol=0)


def _truth_field(F, cs, dists, true_shift, seed):
    rng = np.random.default_rng(seed)
    stamps = np.array([_gauss(cs, rng.uniform(1.8, 3.0), rng.uniform(2, 8), rng.uniform(-0.3, 0.3),
                              rng.uniform(-1, 1, size=2)) for _ in dists])
    field = np.zeros((F, F))
    for st, d, s in zip(stamps, dists, true_shift):
        field += scipy.ndimage.shift(_pad(st, F), shift=(d[0] + s[0], d[1] + s[1]))
    return field, stamps


def test_known_truth_is_recovered():
    F, cs = 259, 25
    g = np.array([-84.0, 0.0, 84.0])
    dists = np.array([[a, b] for a in g for b in g])
    rng = np.random.default_rng(3)
    true_shift = rng.uniform(-2.5, 2.5, size=(len(dists), 2))
    field, stamps = _truth_field(F, cs, dists, true_shift, 4)
    r = _ctx().scene_fit_shifts(field, stamps, dists)
    np.testing.assert_allclose(r["shifts"], true_shift, rtol=0, atol=1e-6)
    assert (r["status"] == 0).all() and (r["iters"] > 0).all(), r
    # an optimum outside the box ends on the bound
    field, stamps = _truth_field(F, cs, [[10.0, -20.0]], [[3.5, -0.4]], 5)
    r = _ctx().scene_fit_shifts(field, stamps, [[10.0, -20.0]], bound=3.0)
    assert r["shifts"][0, 0] == 3.0 and abs(r["shifts"][0, 1] + 0.4) < 0.05, r
    assert r["status"][0] == _ctx().FIT_ON_BOUND


def test_single_and_batch_forms_agree():
    from debvader_amd.deblend_cutout.optimization import position_optimization, position_optimization_batch

    z = np.load(os.path.join(HERE, "golden", "posfit.npz"))
    field = _bands(z["syn_field_r"], 6)
    stamps = _bands(z["syn_stamps_r"], 6)
    F = field.shape[0]
    batch = position_optimization_batch(field, stamps, z["syn_dist"])
    for i, d in enumerate(z["syn_dist"]):
        padded = np.zeros((F, F, 6))
        po = int((F - stamps.shape[1]) / 2)
        padded[po:po + stamps.shape[1], po:po + stamps.shape[1]] = stamps[i]
        sx, sy = position_optimization(field, padded, d)
        np.testing.assert_allclose([sx, sy], batch[i], rtol=0, atol=1e-9)


def test_batches_are_reproducible_and_independent_of_grouping():
    rng = np.random.default_rng(9)
    F, cs, n = 259, 59, 600
    field = rng.normal(0, 0.2, size=(F, F))
    stamps = np.array([_gauss(cs, rng.uniform(2, 4), rng.uniform(1, 5), rng.uniform(-0.3, 0.3)) for _ in range(n)])
    dist = rng.integers(-90, 91, size=(n, 2)).astype(np.float64)
    dist[::7] += 0.5                                   # some fractional distances
    ctx = _ctx()
    a = ctx.scene_fit_shifts(field, stamps, dist)
    b = ctx.scene_fit_shifts(field, stamps, dist)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    for lo in range(0, n, 37):
        part = ctx.scene_fit_shifts(field, stamps[lo:lo + 37], dist[lo:lo + 37])
        for k in a:
            np.testing.assert_array_equal(part[k], a[k][lo:lo + 37])


def test_optimise_positions_end_to_end():
    from debvader_amd.data import synthetic_stamps
    from debvader_amd.deblend.field_deblender import DeblendField
    from debvader_amd.deblend_cutout.optimization import position_optimization_batch
    from debvader_amd.model.model import create_model_vae

    net, _, _, _ = create_model_vae((59, 59, 6), 32, [32, 64, 128, 256], [3, 3, 3, 3])
    rng = np.random.default_rng(2)
    F = 259
    field = rng.normal(0, 0.05, size=(1, F, F, 6))
    x, _ = synthetic_stamps(3, seed=4)
    dists = [[-60, 40], [0, 0], [70, -75]]
    for (dx, dy), s in zip(dists, x):
        field[0, F // 2 + dx - 28:F // 2 + dx + 31, F // 2 + dy - 30:F // 2 + dy + 29] += s   # one pixel off
    db = DeblendField(net, field)
    res = db.deblend_field(dists)
    stamps = np.array([np.asarray(r, np.float64) for r in res["output_images_mean"]])
    expect = position_optimization_batch(field, stamps, np.array(dists, np.float64))
    out = db.optimise_positions()
    assert out is res
    for i in range(len(res)):
        assert isinstance(res["shifts"][i], np.ndarray) and res["shifts"][i].dtype == np.float64
        np.testing.assert_array_equal(res["shifts"][i], expect[i])
    pos = np.array(dists, np.float64) + expect
    np.testing.assert_allclose(db.get_residual_field()[0], so.residual_field(field[0], stamps, pos, 59), rtol=0, atol=1e-9)
    np.testing.assert_allclose(db.get_predicted_field()["predicted_mean_field"], so.predicted_field(F, 6, stamps, pos, 59),
                               rtol=0, atol=1e-9)
    # the on-device path carries no stamps
    dev = DeblendField(net, field)
    rec = dev.deblend_field(dists, on_device=True)
    with pytest.raises(ValueError):
        dev.optimise_positions(rec)
    with pytest.raises(NotImplementedError, match="optimise_positions"):
        db.deblend_field(dists, optimise_positions=True)
