"""The non-negative flux fit without a GPU: the definition on the numpy restatement of
tests/fit_flux_nonneg_oracle.py - the three-Gaussian example, the Karush-Kuhn-Tucker conditions on noisy scenes with spurious
detections, agreement with scipy's NNLS and BVLS, the free sky, the bit-identity of a feasible unconstrained fit, the frozen
statuses, the iteration cap - and the host layer (measurement.fit_nonneg_records / fit_fluxes_nonneg,
DeblendFieldBatch.deblend_fields(fit_nonneg=True), the engine wrappers and the ctypes signatures) over the stand-ins of
tests/stub_fit_flux_nonneg_engine.py."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest

from tests import fit_flux_nonneg_oracle as fn
from tests import fit_flux_oracle as fo
from tests import fit_flux_sky_oracle as fs
from tests.stub_fit_flux_nonneg_engine import (CS, KEYS, NB, NONNEG_FIELD_KEYS, NONNEG_KEYS, SKY_KEYS, WKEYS, Net, OracleContext,
                                               stub_nonneg)
from tests.stub_fit_flux_sky_engine import stub_sky
from tests.stub_fit_flux_weighted_engine import stub_fit_flux_weighted
from tests.stub_measure_engine import stub_catalogue
from tests.test_fit_flux_host import CS31, F64, M1, M2, O1, O2, _c_types, _paste, _stamp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M3, O3 = (3.0, 0.4, 4.5), (0.1, 0.25)


def _triple():
    """three noise-free Gaussians that overlap, cs = 31, F = 64; D = P1 + P2 - 0.1 P3"""
    P = np.stack([_stamp(M1, O1), _stamp(M2, O2, amp=1.7), _stamp(M3, O3, amp=0.8)])
    places = np.array([[16, 14], [16, 20], [19, 17]])
    return P, places, _paste(F64, P, places, amps=[1.0, 1.0, -0.1])


def test_three_gaussians_the_negative_one_is_clamped_and_the_pair_is_refitted():
    P, places, D = _triple()
    free, _ = fo.fit_flux(P, places, [0, 3], D[None])
    assert np.abs(free["fit_scale"] - [[1.0], [1.0], [-0.1]]).max() < 1e-10          # the linear fit returns the negative one
    got, fields = fn.fit_flux_nonneg(P, places, [0, 3], D[None])
    assert (got["fit_scale"][2] == 0.0).all() and not np.signbit(got["fit_scale"][2]).any()
    assert got["fit_clamped"].tolist() == [[0] * 3, [0] * 3, [1] * 3] and got["fit_clamped"].dtype == np.int32
    assert np.array_equal(got["fit_scale_free"], free["fit_scale"])
    assert (got["nonneg_iters"] == 2).all() and (got["nonneg_status"] == 0).all()
    pair, _ = fo.fit_flux(P[:2], places[:2], [0, 2], D[None])
    for b in range(3):                                                               # the 2 x 2 closed form of the pair on D
        G, h = fields[0]["A"][b], fields[0]["rhs"][:, b]
        det = G[0, 0] * G[1, 1] - G[1, 0] * G[1, 0]
        want = np.array([G[1, 1] * h[0] - G[1, 0] * h[1], G[0, 0] * h[1] - G[1, 0] * h[0]]) / det
        assert np.abs(got["fit_scale"][:2, b] - want).max() < 1e-11
        assert np.abs(got["fit_scale"][:2, b] - pair["fit_scale"][:, b]).max() < 1e-11
    assert (got["fit_dual"][2] > 0.0).all() and (got["fit_dual"][:2] == 0.0).all()
    assert np.isnan(got["fit_var"][2]).all() and np.isfinite(got["fit_var"][:2]).all()
    assert np.array_equal(got["fit_var"][:2], pair["fit_var"])                       # the variance of the last passive set
    # clipping the linear fit afterwards is not the least-squares answer: the neighbours keep their bias
    resid = lambda a: np.sqrt(((D - _paste(F64, P, places, amps=a)) ** 2).sum())     # noqa: E731
    clipped = np.maximum(free["fit_scale"][:, 0], 0.0)
    assert resid(got["fit_scale"][:, 0]) < resid(clipped)
    for k in ("fit_gram", "fit_proj", "fit_status"):
        assert np.array_equal(got[k], free[k]), k


@functools.lru_cache(maxsize=None)
def blob_scene(n, cs, F, nb, seed, noise=0.02, spurious=3, width=3.0):
    """n elliptical blobs of cs px scattered over an F x F field, some over the edges; every `spurious`-th one is left out of D
    (a detection without a source: its amplitude comes out near zero, negative about half the time), the others enter at
    amplitudes 0.5 .. 1.5; Gaussian noise on top.  width: the second moments of the blobs in units of those of the crowded field
    of tests/test_gpu_fit_flux.py - at 3 a blob reaches well into its neighbours, and the iteration takes several exchanges.
    Returns (stamps float32, places int32, D (F, F, nb)); never written to."""
    rng = np.random.default_rng(seed)
    s = cs / 31.0
    stamps = np.zeros((n, cs, cs, nb), np.float32)
    for i in range(n):
        a, b = rng.uniform(1.5, 5.0, size=2) * s * s * width
        M = (a, rng.choice([-1.0, 1.0]) * rng.uniform(0.1, 0.6) * np.sqrt(a * b), b)
        p = fo.elliptical_gaussian(cs, M, rng.uniform(-2.0, 2.0, size=2) * s, rng.uniform(0.5, 3.0))
        stamps[i] = (p[:, :, None] * rng.uniform(0.3, 2.0, size=nb)).astype(np.float32)
    # on a jittered grid that overhangs the field: neighbours overlap, nobody coincides
    side = int(np.ceil(np.sqrt(n)))
    cells = rng.permutation(side * side)[:n]
    step = (F - cs // 2) / side
    places = np.stack([(cells // side) * step - cs // 4 + rng.uniform(-0.2, 0.2, n) * step,
                       (cells % side) * step - cs // 4 + rng.uniform(-0.2, 0.2, n) * step], axis=1).astype(np.int32)
    amps = np.where(np.arange(n) % spurious == spurious - 1, 0.0, rng.uniform(0.5, 1.5, size=n)) if spurious else \
        rng.uniform(0.5, 1.5, size=n)
    D = _paste(F, stamps, places, amps=amps) + rng.normal(0.0, noise, size=(F, F, nb))
    for a in (stamps, places, D):
        a.flags.writeable = False
    return stamps, places, D


def _kkt(s, n):
    """the Karush-Kuhn-Tucker conditions of the solve `s` of one band: a >= 0, y >= 0 on Z, and the stationarity of the passive
    set within section 7q's backward bound"""
    P, Z = s["passive"], np.flatnonzero(s["clamped"])
    a = s["scale"]
    assert (a[P[P < n]] >= 0.0).all() and (a[Z] == 0.0).all() and (s["dual"][Z] >= 0.0).all()
    hp = np.zeros(len(a))
    hp[s["kept"]] = s["hp"]
    if len(P):
        A = s["full"][np.ix_(P, P)]
        back = np.abs(A @ a[P] - hp[P]).max()
        assert back <= 1e-10 * (np.abs(A).sum(axis=1).max() * np.abs(a[P]).max() + np.abs(hp[P]).max())
    for i in Z:                                                      # the dual is the gradient of the clamped galaxy
        assert abs(s["dual"][i] - (s["full"][i, P] @ a[P] - hp[i])) <= 1e-10 * (np.abs(s["full"][i, P] * a[P]).sum() + abs(hp[i]))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_kkt_and_scipy_on_noisy_scenes_with_spurious_detections(seed):
    import scipy.optimize as so

    n = 40
    stamps, places, D = blob_scene(n, 15, 64, 2, seed)
    for order in (None, 0, 1):
        got, fields = fn.fit_flux_nonneg(stamps, places, [0, n], D[None], order)
        q = 0 if order is None else fs.sky_terms(order)
        assert (got["nonneg_status"] == 0).all() and (got["nonneg_iters"] >= 2).all() and (got["nonneg_iters"] <= 8).all()
        assert got["fit_clamped"].sum() >= 3 and (got["fit_scale_free"][got["fit_clamped"] == 1] < 0.0).any()
        for b, s in enumerate(fields[0]["bands"]):
            _kkt(s, n)
            assert s["sizes"][-1] == 0 and len(s["sizes"]) == s["iters"]
            kept, hp = s["kept"], s["hp"]
            L = np.linalg.cholesky(s["full"][np.ix_(kept, kept)])
            rhs = np.linalg.solve(L, hp)
            a = s["scale"][kept]
            if q == 0:
                want, _ = so.nnls(L.T, rhs)
            else:                                                    # the sky bounds infinite
                lo = np.where(kept < n, 0.0, -np.inf)
                want = so.lsq_linear(L.T, rhs, bounds=(lo, np.full(len(kept), np.inf)), method="bvls", tol=1e-14).x
            assert np.abs(a - want).max() <= 1e-10 * np.abs(a).max(), (order, b, np.abs(a - want).max())
            assert np.array_equal(want[kept < n] == 0.0, s["clamped"][kept[kept < n]] == 1)


def test_a_negative_sky_is_fitted_and_never_clamped():
    n = 12
    stamps, places, D = blob_scene(n, 15, 48, 1, seed=5, spurious=0)
    for order in (0, 1):
        got, fields = fn.fit_flux_nonneg(stamps, places, [0, n], (D - 0.05)[None], order)
        assert (got["sky_status"] == 0).all() and np.abs(got["sky_coef"][0, :, 0] + 0.05).max() < 0.01      # negative, to the noise
        assert (got["sky_coef"][0, :, 0] < 0.0).all() and (got["fit_clamped"] == 0).all() and (got["nonneg_iters"] == 1).all()
        assert all(s["clamped"][n:].sum() == 0 for s in fields[0]["bands"])
    # ... with spurious detections beside it the sky stays free while galaxies are clamped
    stamps, places, D = blob_scene(n, 15, 48, 1, seed=5)
    got, _ = fn.fit_flux_nonneg(stamps, places, [0, n], (D - 0.05)[None], 0)
    assert got["fit_clamped"].sum() >= 1 and (got["sky_coef"] < 0.0).all() and (got["nonneg_status"] == 0).all()


def test_an_all_positive_scene_has_the_arrays_of_the_unconstrained_fit():
    n = 12
    stamps, places, D = blob_scene(n, 15, 48, 2, seed=7, spurious=0)
    want, _ = fo.fit_flux(stamps, places, [0, n], D[None])
    assert (want["fit_scale"] > 0.0).all()
    got, _ = fn.fit_flux_nonneg(stamps, places, [0, n], D[None])
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["fit_scale_free"], want["fit_scale"]) and (got["fit_clamped"] == 0).all()
    assert (got["fit_dual"] == 0.0).all() and (got["nonneg_iters"] == 1).all() and (got["nonneg_status"] == 0).all()
    W = np.random.default_rng(2).uniform(0.5, 2.0, size=D.shape)
    for order in (0, 1):
        want, _ = fs.fit_flux_sky(stamps, places, [0, n], D[None], order, W[None])
        got, _ = fn.fit_flux_nonneg(stamps, places, [0, n], D[None], order, W[None])
        for k in WKEYS + SKY_KEYS:
            assert np.array_equal(got[k], want[k], equal_nan=True), (order, k)
        assert (got["nonneg_iters"] == 1).all()
    # a field without unknowns: no factorisation; without galaxies but with a sky: one
    none = np.zeros((0, 15, 15, 2), np.float32)
    got, _ = fn.fit_flux_nonneg(none, np.zeros((0, 2)), [0, 0], D[None])
    assert (got["nonneg_iters"] == 0).all() and (got["nonneg_status"] == 0).all()
    got, _ = fn.fit_flux_nonneg(none, np.zeros((0, 2)), [0, 0], D[None], 1)
    assert (got["nonneg_iters"] == 1).all() and (got["sky_status"] == 0).all()


def test_a_duplicate_behind_a_clamped_galaxy_keeps_its_status():
    P = np.stack([_stamp(M1, O1), _stamp(M2, O2, amp=1.7), _stamp(M2, O2, amp=1.7), np.zeros((CS31, CS31, 3), np.float32)])
    places = np.array([[16, 14], [16, 20], [16, 20], [30, 30]])
    D = _paste(F64, P[:2], places[:2], amps=[1.0, 0.5])                  # the duplicate keeps amplitude 1: 0.5 - 1 is left for P2
    free, _ = fo.fit_flux(P, places, [0, 4], D[None])
    assert free["fit_status"].tolist() == [[0] * 3, [0] * 3, [5] * 3, [4] * 3]
    assert np.abs(free["fit_scale"][:3] - [[1.0], [-0.5], [1.0]]).max() < 1e-10
    got, _ = fn.fit_flux_nonneg(P, places, [0, 4], D[None])
    assert np.array_equal(got["fit_status"], free["fit_status"]) and got["fit_clamped"].tolist() == [[0] * 3, [1] * 3, [0] * 3, [0] * 3]
    assert (got["fit_scale"][1] == 0.0).all() and (got["fit_scale"][2] == 1.0).all() and np.isnan(got["fit_scale"][3]).all()
    assert np.isnan(got["fit_dual"][2:]).all() and (got["fit_dual"][1] > 0.0).all() and (got["fit_dual"][0] == 0.0).all()
    assert np.isnan(got["fit_var"][1:]).all() and np.array_equal(got["fit_scale_free"], free["fit_scale"], equal_nan=True)
    assert (got["nonneg_iters"] == 2).all()


def test_max_iter_one_returns_the_free_fit_and_says_so():
    P, places, D = _triple()
    free, _ = fo.fit_flux(P, places, [0, 3], D[None])
    got, _ = fn.fit_flux_nonneg(P, places, [0, 3], D[None], max_iter=1)
    assert (got["nonneg_status"] == 1).all() and (got["nonneg_iters"] == 1).all() and (got["fit_clamped"] == 0).all()
    for k in KEYS:
        assert np.array_equal(got[k], free[k]), k
    assert (got["fit_scale"][2] < 0.0).all() and (got["fit_dual"] == 0.0).all()
    with pytest.raises(AssertionError):
        fn.solve_band_nonneg(np.eye(2), np.ones(2), 2, max_iter=0)


def test_fit_nonneg_records_and_fit_fluxes_nonneg():
    from debvader_amd.measure import measurement as ms

    assert [d[0] for d in ms.fit_nonneg_dtype(3)] == ["fit_scale_free", "flux_fit_free", "fit_clamped", "fit_dual"]
    assert ms.fit_nonneg_dtype(3)[2] == ("fit_clamped", "<i4", (3,))
    rec = ms.fit_nonneg_records([[-0.5, np.nan]], [[1, 0]], [[2.0, np.nan]], [[10.0, 20.0]])
    assert rec["flux_fit_free"][0, 0] == -5.0 and np.isnan(rec["flux_fit_free"][0, 1]) and rec["fit_clamped"].tolist() == [[1, 0]]
    with pytest.raises(ValueError, match="expected flux"):
        ms.fit_nonneg_records(np.zeros((2, 3)), np.zeros((2, 3)), np.zeros((2, 3)), np.zeros((2, 2)))
    with pytest.raises(ValueError, match="expected fit_scale_free"):
        ms.fit_nonneg_records(np.zeros(3), np.zeros(3), np.zeros(3), np.zeros(3))
    P, places, D = _triple()
    ctx = OracleContext()
    flux = P.sum(axis=(1, 2), dtype=np.float64)
    for W in (None, np.full_like(D, 4.0)):
        for order in (None, 0, 1):
            sigma = None if W is not None else np.full(3, 0.5)
            cat, per_field = ms.fit_fluxes_nonneg(P, places, D, sky_order=order, weight_fields=W, sky_sigma=sigma, ctx=ctx)
            base = ms.fit_flux_dtype(3) if W is None else ms.fit_flux_weighted_dtype(3)
            want = base + ([] if order is None else ms.fit_sky_dtype(3)) + ms.fit_nonneg_dtype(3)
            assert cat.dtype == np.dtype(want) and len(cat) == 3                      # the new columns come last
            assert list(per_field) == list(NONNEG_FIELD_KEYS + (() if order is None else SKY_KEYS))
            assert per_field["nonneg_iters"].shape == (1, 3) and per_field["nonneg_iters"].dtype == np.int32
            assert ctx.calls[-1]["fit_flux_nonneg"] == 3 and ctx.calls[-1]["sky_order"] == order and ctx.calls[-1]["max_iter"] == 100
            assert (cat["fit_clamped"][2] == 1).all() and (cat["fit_scale"][2] == 0.0).all() and (cat["flux_fit"][2] == 0.0).all()
            assert np.abs(cat["fit_scale_free"][2] + 0.1).max() < 1e-9
            assert np.array_equal(cat["flux_fit_free"], cat["fit_scale_free"] * flux)
            # a NaN fit_var makes the derived columns of a clamped galaxy NaN - and only those
            for k in ("fit_var", "fit_scale_err", "flux_fit_err", "fit_independence"):
                assert np.isnan(cat[k][2]).all() and np.isfinite(cat[k][:2]).all(), k
            assert np.isfinite(cat["fit_scale_alone"]).all() and (cat["fit_dual"][2] > 0).all()
    cat, _ = ms.fit_fluxes_nonneg(P, places, D, max_iter=1, ctx=ctx)
    assert ctx.calls[-1]["max_iter"] == 1 and (cat["fit_clamped"] == 0).all() and (cat["fit_scale"][2] < 0).all()
    before = len(ctx.calls)
    for kw, match in ((dict(sky_order=2), "sky_order must be 0"), (dict(sky_order=True), "sky_order must be 0"),
                      (dict(sky_order=-1), "sky_order must be 0"),
                      (dict(max_iter=0), "max_iter must be an integer >= 1"), (dict(max_iter=2.5), "max_iter must be an integer >= 1"),
                      (dict(max_iter=True), "max_iter must be an integer >= 1"),
                      (dict(weight_fields=np.ones_like(D), sky_sigma=np.ones(3)), "weights already carry the noise"),
                      (dict(weight_fields=np.ones((F64, F64, 2))), "expected weight fields of the shape of the data fields"),
                      (dict(sky_sigma=np.ones(4)), "sky_sigma"),
                      (dict(catalogue=np.recarray((3,), dtype=[("x", "<f8")])), "lacks the column flux")):
        with pytest.raises(ValueError, match=match):
            ms.fit_fluxes_nonneg(P, places, D, ctx=ctx, **kw)
    assert len(ctx.calls) == before
    assert list(inspect.signature(ms.fit_fluxes_nonneg).parameters) == [
        "stamps_mean", "places", "data_fields", "sky_order", "weight_fields", "field_ptr", "catalogue", "sky_sigma", "min_pivot",
        "max_iter", "ctx"]
    p = inspect.signature(ms.fit_fluxes_nonneg).parameters
    assert p["sky_order"].default is None and p["max_iter"].default == 100 and p["min_pivot"].default == 1e-8


F = 81
DIST = [np.array([[0.0, 0.0], [5.0, -7.0]]), np.zeros((0, 2)), np.array([[100.0, 0.0], [-3.0, 11.0]]), np.array([[0.0, 40.0]])]


def _batch():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch

    net = Net()
    return net, DeblendFieldBatch(net, np.random.default_rng(3).normal(size=(4, F, F, NB)), CS, NB)


def _engine_calls(net):
    return [c for c in net._core.engine.calls if c[0].startswith("infer")]


def test_deblend_fields_appends_the_nonneg_columns_last_and_keeps_the_field_arrays():
    from debvader_amd.deblend.field_deblender import _EXTRAS, DeblendFieldBatch
    from debvader_amd.measure import measurement as ms

    sig = inspect.signature(DeblendFieldBatch.deblend_fields).parameters
    assert sig["fit_nonneg"].default is False and sig["fit_nonneg"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(sig)[-4:] == ["fit_weights", "fit_nonneg", "fit_sky", "optimise_positions"]
    assert _EXTRAS[-1].key == "fit_nonneg" and _EXTRAS[-1].refines == "fit_flux"
    assert DeblendFieldBatch.fit_nonneg_columns(NB) == ms.fit_nonneg_dtype(NB)
    net, b = _batch()
    assert b.nonneg_fit is None
    W = np.random.default_rng(5).uniform(0.5, 2.0, size=(4, F, F, NB))
    places = (int((F - CS) / 2) + np.array([[0, 0], [5, -7], [-3, 11]])).astype(np.int64)      # the three galaxies that pass the border cut
    for weights in (None, W):
        fit_cols = DeblendFieldBatch.fit_flux_columns(NB) if weights is None else DeblendFieldBatch.fit_flux_weighted_columns(NB)
        for order in (None, 0, 1):
            want = np.dtype(DeblendFieldBatch.ON_DEVICE_COLUMNS + DeblendFieldBatch.measure_columns(NB) + fit_cols +
                            ([] if order is None else DeblendFieldBatch.fit_sky_columns(NB)) + DeblendFieldBatch.fit_nonneg_columns(NB))
            for rf in (True, False):
                sky_sigma = None if weights is not None else np.full(NB, 0.3)
                res = b.deblend_fields(DIST, on_device=True, measure=True, fit_flux=True, fit_nonneg=True, fit_sky=order,
                                       fit_weights=weights, sky_sigma=sky_sigma, return_fields=rf)
                (call,) = _engine_calls(net)[-1:]
                assert call[0] == "infer_fields_measure_fit_nonneg" and call[2] is rf and np.array_equal(call[3], places)
                assert call[4] == order and (call[5] is None if weights is None else np.array_equal(call[5], W)) and call[6] == 100
                assert [len(r) for r in res] == [2, 0, 1, 0] and all(r.dtype == want for r in res)
                f, c = stub_fit_flux_weighted(3, NB), stub_catalogue(3, NB)
                nn = stub_nonneg(f, 4, NB)
                assert nn["fit_clamped"].sum() == 1                                   # the stub clamps galaxy 2 in band 1
                if weights is None:
                    cat = ms.fit_flux_records(*(f[k] for k in KEYS), c["flux"], sky_sigma=sky_sigma, field_ptr=[0, 2, 2, 3, 3])
                else:
                    cat = ms.fit_flux_records(*(f[k] for k in KEYS), c["flux"], fit_chi2=f["fit_chi2"], fit_npix=f["fit_npix"])
                parts = [cat, ms.fit_nonneg_records(*(nn[k] for k in NONNEG_KEYS), c["flux"])]
                if order is not None:
                    sky = stub_sky(4, NB, 1 if order == 0 else 3, F)
                    parts.append(ms.fit_sky_records(sky["sky_coef"], sky["sky_cov"], sky["sky_status"], places, CS, F,
                                                    field_ptr=[0, 2, 2, 3, 3], sky_sigma=sky_sigma, weighted=weights is not None))
                    assert list(b.sky_fit) == list(SKY_KEYS)
                else:
                    assert b.sky_fit is None
                for i, (m, k) in enumerate([(0, 0), (0, 1), (2, 0)]):
                    for part in parts:
                        for name in part.dtype.names:
                            assert np.array_equal(res[m][name][k], part[name][i], equal_nan=True), name
                assert res[2]["fit_clamped"][0, 1] == 1 and res[2]["fit_scale"][0, 1] == 0.0 and res[2]["flux_fit"][0, 1] == 0.0
                assert np.isnan(res[2]["fit_scale_err"][0, 1]) and np.isnan(res[2]["fit_independence"][0, 1])
                assert list(b.nonneg_fit) == list(NONNEG_FIELD_KEYS)
                for k in NONNEG_FIELD_KEYS:
                    assert np.array_equal(b.nonneg_fit[k], nn[k]) and b.nonneg_fit[k].shape == (4, NB)
    # without fit_nonneg the calls, the columns and the attribute are those of before
    res = b.deblend_fields(DIST, on_device=True, measure=True, fit_flux=True)
    assert _engine_calls(net)[-1][0] == "infer_fields_measure_fit" and "fit_clamped" not in res[0].dtype.names and b.nonneg_fit is None
    res = b.deblend_fields(DIST, on_device=True, measure=True, fit_flux=True, fit_weights=W)
    assert _engine_calls(net)[-1][0] == "infer_fields_measure_fit_weighted" and "fit_clamped" not in res[0].dtype.names
    res = b.deblend_fields(DIST, on_device=True, measure=True, fit_flux=True, fit_sky=1)
    assert _engine_calls(net)[-1][0] == "infer_fields_measure_fit_sky" and "fit_clamped" not in res[0].dtype.names


def test_deblend_fields_refuses_fit_nonneg_combinations():
    net, b = _batch()
    W = np.ones((4, F, F, NB))
    on = dict(on_device=True, measure=True)
    for kw, match in ((dict(fit_nonneg=True, **on), "fit_nonneg=True needs fit_flux=True"),
                      (dict(fit_nonneg=True), "fit_nonneg=True needs fit_flux=True"),
                      (dict(fit_nonneg=True, fit_weights=W, **on), "needs fit_flux=True"),
                      (dict(fit_nonneg=True, fit_sky=0, **on), "needs fit_flux=True"),
                      # every refusal of fit_flux stays
                      (dict(fit_nonneg=True, fit_flux=True), "fit_flux=True needs measure=True and on_device=True"),
                      (dict(fit_nonneg=True, fit_flux=True, measure=True), "fit_flux=True needs measure=True and on_device=True"),
                      (dict(fit_nonneg=True, fit_flux=True, on_device=True), "fit_flux=True needs measure=True and on_device=True"),
                      (dict(fit_nonneg=True, fit_flux=True, fit_sky=2, **on), "sky_order must be 0"),
                      (dict(fit_nonneg=True, fit_flux=True, psf=np.ones((21, 21)), **on), "fit_flux=True cannot be combined with psf"),
                      (dict(fit_nonneg=True, fit_flux=True, apertures=(3.0,), **on), "fit_flux=True cannot be combined with apertures"),
                      (dict(fit_nonneg=True, fit_flux=True, blendedness=True, **on), "fit_flux=True cannot be combined with blendedness"),
                      (dict(fit_nonneg=True, fit_flux=True, measure_samples=4, **on),
                       "fit_flux=True cannot be combined with measure_samples"),
                      (dict(fit_nonneg=True, fit_flux=True, optimise_positions=True, **on),
                       "fit_flux=True cannot be combined with optimise_positions"),
                      (dict(fit_nonneg=True, fit_flux=True, epistemic_uncertainty_estimation=True, **on),
                       "fit_flux=True cannot be combined with epistemic_uncertainty_estimation"),
                      (dict(fit_nonneg=True, fit_flux=True, fit_weights=W, sky_sigma=np.ones(NB), **on), "weights already carry the noise"),
                      (dict(fit_nonneg=True, fit_flux=True, fit_weights=W[:3], **on),
                       "expected weight fields of the shape of the data fields")):
        with pytest.raises(ValueError, match=match):
            b.deblend_fields(DIST, **kw)
    assert not _engine_calls(net) and net._core.seed_counter == 7


def test_engine_wrappers_refuse_before_the_library():
    from debvader_amd import engine as E

    assert E.nonneg_max_iter(1) == 1 and E.nonneg_max_iter(np.int64(7)) == 7
    assert E.FIT_NONNEG_KEYS == NONNEG_KEYS and E.FIT_NONNEG_FIELD_KEYS == NONNEG_FIELD_KEYS
    P, pl, D = np.zeros((2, 31, 31, 3), np.float32), np.zeros((2, 2), np.int32), np.zeros((1, 40, 40, 3))
    call = lambda *a, **kw: E.Context.scene_fit_flux_nonneg(object(), *a, **kw)     # noqa: E731
    for kw, match in ((dict(sky_order=2), "sky_order must be 0"), (dict(sky_order=-1), "sky_order must be 0"),
                      (dict(max_iter=0), "max_iter must be an integer >= 1"), (dict(max_iter=1.5), "max_iter must be an integer >= 1"),
                      (dict(weight_fields=np.zeros((1, 40, 40, 2))), "expected weight fields of the shape of the data fields"),
                      (dict(min_pivot=0.0), "min_pivot"), (dict(scratch_bytes=0), "scratch_bytes"),
                      (dict(field_ptr=[0, 1]), "field_ptr")):
        with pytest.raises(ValueError, match=match):
            call(P, pl, D, **kw)
    with pytest.raises(ValueError, match="expected data fields"):
        call(P, pl, D[0])
    with pytest.raises(ValueError, match="expected places"):
        call(P, pl[:1], D)
    fields = np.zeros((2, 81, 81, 6))
    for kw, match in ((dict(places=None), "places are needed"), (dict(places=None, return_fields=False), "places are needed"),
                      (dict(places=[[0, 0]], sky_order=2), "sky_order must be 0"),
                      (dict(places=[[0, 0]], fit_max_iter=0), "max_iter must be an integer >= 1"),
                      (dict(places=[[0, 0]], weight_fields=fields[:1]), "expected weight fields of the shape of the data fields"),
                      (dict(places=[[0, 0]], min_pivot=2.0), "min_pivot"), (dict(places=[[0, 0]], band=7), "band")):
        places = kw.pop("places")
        with pytest.raises(ValueError, match=match):
            E.Engine.infer_fields_measure_fit_nonneg(object(), fields, [[0, 0]], [0, 1, 1], places, **kw)
    out, ptrs = E._fit_nonneg_out(5, 4, 6)
    assert list(out) == list(NONNEG_KEYS + NONNEG_FIELD_KEYS) and len(ptrs) == 5
    assert out["fit_scale_free"].shape == (5, 6) and out["fit_clamped"].dtype == np.int32 and out["fit_dual"].dtype == np.float64
    assert out["nonneg_iters"].shape == (4, 6) and out["nonneg_iters"].dtype == np.int32 and out["nonneg_status"].dtype == np.int32
    sky, order, sky_ptrs = E._fit_sky_args(None, 4, 6)
    assert sky == {} and order == -1 and sky_ptrs == [None] * 4
    sky, order, sky_ptrs = E._fit_sky_args(1, 4, 6)
    assert list(sky) == list(SKY_KEYS) and order == 1 and sky["sky_coef"].shape == (4, 6, 3)
    # a call without fields returns without the library; the keys and their order
    empty = call(P[:0], pl[:0], D[:0], field_ptr=[0])
    assert list(empty) == list(KEYS + NONNEG_KEYS + NONNEG_FIELD_KEYS) and empty["nonneg_iters"].shape == (0, 3)
    assert list(call(P[:0], pl[:0], D[:0], field_ptr=[0], weight_fields=D[:0], sky_order=1)) == \
        list(WKEYS + SKY_KEYS + NONNEG_KEYS + NONNEG_FIELD_KEYS)
    for name in ("infer_fields_measure_fit_nonneg", "infer_cutouts_measure_fit_nonneg", "scene_fit_flux_nonneg"):
        assert hasattr(E.Engine, name), name
    assert "weight_field" in inspect.signature(E.Engine.infer_cutouts_measure_fit_nonneg).parameters
    # the existing calls keep their parameter lists
    p = inspect.signature(E.Context.scene_fit_flux_sky).parameters
    assert "max_iter" not in p and p["sky_order"].default == 0
    assert "fit_max_iter" not in inspect.signature(E.Engine.infer_fields_measure_fit_sky).parameters


def test_header_binding_and_library_agree_on_the_nonneg_entry_points():
    from debvader_amd import _lib

    header = open(os.path.join(ROOT, "include", "debvader_hip.h")).read()
    ctype = {"dv_model*": C.c_void_p, "dv_ctx*": C.c_void_p, "double*": C.POINTER(C.c_double), "float*": C.POINTER(C.c_float),
             "int32_t*": C.POINTER(C.c_int32), "int64_t*": C.POINTER(C.c_int64), "int32_t": C.c_int32, "int64_t": C.c_int64,
             "uint64_t": C.c_uint64, "double": C.c_double, "dv_measure_params*": C.POINTER(_lib.DvMeasureParams),
             "dv_fit_flux_params*": C.POINTER(_lib.DvFitFluxParams)}
    for name, nargs in (("dv_scene_fit_flux_nonneg", 30), ("dv_infer_fields_measure_fit_nonneg", 40)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header, re.S)
        assert m, f"{name} is not declared in include/debvader_hip.h"
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)         # bound: the library exports it
        restype, argtypes = _lib.SIGNATURES[name]
        want = [ctype[t] for t in _c_types(m.group(1))]
        assert restype is C.c_int and len(argtypes) == len(want) == nargs
        for i, (a, w) in enumerate(zip(argtypes, want)):
            assert a is w, (name, i, a, w)
        assert getattr(_lib.lib, name).argtypes == argtypes
        names = [re.sub(r".*?(\w+)$", r"\1", a.strip()) for a in m.group(1).split(",")]
        assert names[-5:] == ["fit_scale_free", "fit_clamped", "fit_dual", "nonneg_iters", "nonneg_status"]
        assert names[names.index("sky_order") + 1] == "max_iter"
    # the sky calls' arguments up to sky_order, max_iter behind it, their outputs, and the five new outputs last
    new_out = [C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    sn, ss = _lib.SIGNATURES["dv_scene_fit_flux_nonneg"][1], _lib.SIGNATURES["dv_scene_fit_flux_sky"][1]
    assert sn[:13] == ss[:13] and sn[13] is C.c_int32 and sn[14:25] == ss[13:] and sn[25:] == new_out
    pn, ps = _lib.SIGNATURES["dv_infer_fields_measure_fit_nonneg"][1], _lib.SIGNATURES["dv_infer_fields_measure_fit_sky"][1]
    assert pn[:23] == ps[:23] and pn[23] is C.c_int32 and pn[24:35] == ps[23:] and pn[35:] == new_out
    # the existing entry points keep their argument counts, and the parameter struct its two fields
    for name, nargs in (("dv_scene_fit_flux", 16), ("dv_infer_fields_measure_fit", 26), ("dv_scene_fit_flux_gram", 10),
                        ("dv_scene_fit_flux_weighted", 19), ("dv_infer_fields_measure_fit_weighted", 29),
                        ("dv_scene_fit_flux_sky", 24), ("dv_infer_fields_measure_fit_sky", 34), ("dv_scene_fit_flux_sky_gram", 12),
                        ("dv_fit_flux_params_default", 1)):
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    assert [f[0] for f in _lib.DvFitFluxParams._fields_] == ["min_pivot", "scratch_bytes"]
    kernel = open(os.path.join(ROOT, "debvader_amd", "csrc", "fitflux.hip")).read()
    for k in ("fitflux_nonneg_kernel", "fitflux_solve_kernel", "#pragma clang fp contract(off)"):
        assert k in kernel, k
    assert "getenv" not in kernel and "atomic" not in kernel.split("fitflux_nonneg_kernel(", 1)[1].split("// The chi-square", 1)[0]
    engine = open(os.path.join(ROOT, "debvader_amd", "csrc", "engine.hip")).read()
    assert "dv_infer_fields_measure_fit_nonneg" in engine and "dv_scene_fit_flux_nonneg" in engine
