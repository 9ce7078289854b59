"""CPU checks of the Monte-Carlo catalogue: the numpy restatement of the fold against np.mean / np.std
taken directly, and the Python layer - measure_stamps_mc and DeblendFieldBatch.deblend_fields(measure_samples=S) - over the
stand-in engine of tests/stub_measure_mc_engine.py.  No GPU is touched."""
import inspect
import os
import re

import numpy as np
import pytest

from tests import measure_mc_oracle as mmo
from tests import measure_oracle as mo
from tests.stub_measure_mc_engine import CS, NB, Net, OracleMcContext, stub_mc_catalogue
from tests.stub_measure_engine import stub_catalogue

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MC_KEYS = ("flux_mc_mean", "flux_mc_std", "shape_mc_mean", "shape_mc_std", "n_ok")


def _sample_sets(cs=31, nb=3, S=6):
    """(S, N, cs, cs, nb) float32 and what n_ok must be: jittered Gaussians; all samples zero; one good sample among zeros;
    a spike and a zero among good samples; all samples good but one spike"""
    good = [mmo.jittered_gaussians(cs, nb, S, seed) for seed in range(5)]
    zero, spike = np.zeros((cs, cs, nb), np.float32), mmo.spike_stamp(cs, nb)
    g = [good[0], good[1]]
    g.append(np.stack([zero] * S))
    one = np.stack([zero] * S)
    one[2] = good[2][2]
    g.append(one)
    some = good[3].copy()
    some[1], some[4] = spike, zero
    g.append(some)
    last = good[4].copy()
    last[S - 1] = spike
    g.append(last)
    return np.stack(g, axis=1), [S, S, 0, 1, S - 2, S - 1]


def test_the_fold_against_numpy_mean_and_std():
    samples, n_ok = _sample_sets()
    got = mmo.measure_mc(samples)
    assert got["n_ok"].tolist() == n_ok
    # status per sample as constructed: zero and spike stamps fail, the Gaussians converge
    assert (got["sample_status"][:2] == mo.CONVERGED).all() and (got["sample_status"][2] == mo.FAILED).all()
    assert got["sample_status"][3].tolist() == [3, 3, 0, 3, 3, 3] and got["sample_status"][4].tolist() == [0, 3, 0, 0, 3, 0]
    want = mmo.direct(got["sample_flux"], got["sample_shape"], got["sample_status"])
    assert np.array_equal(got["n_ok"], want["n_ok"])
    for k in MC_KEYS[:4]:
        scale = np.abs(want[k]).max(axis=1, keepdims=True) if k.endswith("mean") else \
            np.abs(want[k.replace("std", "mean")]).max(axis=1, keepdims=True)
        err = np.abs(got[k] - want[k]) / np.where(scale > 0, scale, 1.0)
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), k
        assert np.nanmax(err, initial=0.0) <= 1e-12, (k, np.nanmax(err))
    # the jitter is there: the standard deviations are not rounding noise
    assert (got["shape_mc_std"][0] > 1e-3).all() and (got["flux_mc_std"][0] > 1e-3).all()
    # no accepted sample: NaN; exactly one: its row with a standard deviation of exactly 0; the fluxes count every sample
    assert np.isnan(got["shape_mc_mean"][2]).all() and np.isnan(got["shape_mc_std"][2]).all()
    assert (got["flux_mc_mean"][2] == 0).all() and (got["flux_mc_std"][2] == 0).all()
    row, ok = mmo.shape_row(got["sample_shape"][3, 2], 0)
    assert ok and np.array_equal(got["shape_mc_mean"][3], row) and (got["shape_mc_std"][3] == 0).all()
    assert np.allclose(got["flux_mc_mean"][3], got["sample_flux"][3, 2] / 6.0, rtol=1e-14)


def test_the_fold_does_not_depend_on_how_the_samples_are_split():
    """Welford in sample order: folding passes of 3, 3 and 1 samples from the carried state is folding all 7"""
    rng = np.random.default_rng(5)
    flux, shape = rng.uniform(1, 2, size=(4, 7, 3)), rng.uniform(1, 2, size=(4, 7, 5)) * [1, 1, 4, 0.1, 4]
    status = np.where(rng.random((4, 7)) < 0.3, 3, 0).astype(np.int32)
    whole = mmo.fold(flux, shape, status)
    perm = rng.permutation(4)
    moved = mmo.fold(flux[perm], shape[perm], status[perm])
    for k in MC_KEYS:
        assert np.array_equal(moved[k], whole[k][perm], equal_nan=True), k
    assert np.array_equal(mmo.fold(flux[1:2], shape[1:2], status[1:2])["shape_mc_std"][0], whole["shape_mc_std"][1], equal_nan=True)


def test_measure_stamps_mc_columns_and_argument_checks():
    from debvader_amd import engine as E
    from debvader_amd.measure.measurement import MC_SHAPE_NAMES, catalogue_mc_dtype, measure_stamps_mc

    assert MC_SHAPE_NAMES == mmo.SHAPE_NAMES
    names = [c[0] for c in catalogue_mc_dtype(3)]
    assert names == ["flux_mc_mean", "flux_mc_std"] + [f"{q}_mc_{s}" for q in mmo.SHAPE_NAMES for s in ("mean", "std")] + ["n_ok"]
    assert np.dtype(catalogue_mc_dtype(3))["flux_mc_std"].shape == (3,) and np.dtype(catalogue_mc_dtype(3))["n_ok"] == np.int32
    sig = inspect.signature(measure_stamps_mc).parameters
    assert sig["band"].default == 2 and sig["keep_samples"].default is False and sig["max_iter"].default == 200
    ctx = OracleMcContext()
    samples, n_ok = _sample_sets()
    rec = measure_stamps_mc(samples.astype(np.float64), ctx=ctx)
    assert rec.dtype == np.dtype(catalogue_mc_dtype(3)) and rec.shape == (6,)
    assert ctx.calls[0]["dtype"] == np.float32 and ctx.calls[0]["S"] == 6 and not ctx.calls[0]["keep_samples"]
    ref = mmo.measure_mc(samples)
    assert np.array_equal(rec["n_ok"], ref["n_ok"]) and np.array_equal(rec["flux_mc_std"], ref["flux_mc_std"])
    for k, q in enumerate(mmo.SHAPE_NAMES):
        assert np.array_equal(rec[q + "_mc_mean"], ref["shape_mc_mean"][:, k], equal_nan=True)
        assert np.array_equal(rec[q + "_mc_std"], ref["shape_mc_std"][:, k], equal_nan=True)
    rec2, rows = measure_stamps_mc(samples, keep_samples=True, sigma0=2.5, ctx=ctx)
    assert sorted(rows) == ["sample_flux", "sample_shape", "sample_status"] and rows["sample_shape"].shape == (6, 6, 5)
    assert ctx.calls[-1]["keep_samples"] and ctx.calls[-1]["sigma0"] == 2.5
    n_calls = len(ctx.calls)
    good = np.zeros((2, 2, 31, 31, 3))
    for kw, msg in [(dict(band=3), "band"), (dict(band=-1), "band"), (dict(band=1.5), "band"), (dict(sigma0=0.0), "sigma0"),
                    (dict(tol=float("nan")), "tol"), (dict(max_iter=-1), "max_iter")]:
        with pytest.raises(ValueError, match=msg):
            measure_stamps_mc(good, ctx=ctx, **kw)
    with pytest.raises(ValueError, match="sample stamps"):
        measure_stamps_mc(np.zeros((2, 31, 31, 3)), ctx=ctx)
    with pytest.raises(ValueError, match="sample stamps"):
        measure_stamps_mc(np.zeros((2, 2, 31, 30, 3)), ctx=ctx)
    with pytest.raises(ValueError, match="at least one"):
        measure_stamps_mc(np.zeros((0, 2, 31, 31, 3)), ctx=ctx)
    with pytest.raises(ValueError, match="at most 90"):
        measure_stamps_mc(np.zeros((1, 1, 91, 91, 1)), band=0, ctx=ctx)
    assert len(ctx.calls) == n_calls
    # the engine's wrappers check before they touch the library
    with pytest.raises(ValueError, match="band"):
        E.Context.scene_measure_mc(object(), good, band=5)
    with pytest.raises(ValueError, match="places"):
        E.Engine.infer_fields_measure_mc(object(), np.zeros((1, 81, 81, 6)), [[0, 0]], [0, 1])
    with pytest.raises(ValueError, match="nsamples"):
        E.Engine.infer_fields_measure_mc(object(), np.zeros((1, 81, 81, 6)), [[0, 0]], [0, 1], return_fields=False, nsamples=0)
    with pytest.raises(ValueError, match="max_iter"):
        E.Engine.infer_fields_measure_mc(object(), np.zeros((1, 81, 81, 6)), [[0, 0]], [0, 1], return_fields=False, max_iter=-2)


def test_the_two_symbols_are_declared_and_bound():
    from debvader_amd import _lib

    header = open(os.path.join(ROOT, "include", "debvader_hip.h")).read()
    for name, nargs in (("dv_scene_measure_mc", 15), ("dv_infer_fields_measure_mc", 30)):
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs
        assert len(_lib.SIGNATURES[name][1]) == nargs
        assert hasattr(_lib.lib, name)


F = 81
DIST = [np.array([[0.0, 0.0], [5.0, -7.0]]), np.zeros((0, 2)), np.array([[100.0, 0.0], [-3.0, 11.0]]), np.array([[0.0, 40.0]])]


def _batch():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch

    net = Net()
    return net, DeblendFieldBatch(net, np.random.default_rng(3).normal(size=(4, F, F, NB)), CS, NB)


def test_deblend_fields_measure_samples_on_device():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch

    sig = inspect.signature(DeblendFieldBatch.deblend_fields).parameters
    assert sig["measure_samples"].default == 0 and sig["measure_samples"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(sig)[-1] == "optimise_positions"
    net, b = _batch()
    res = b.deblend_fields(DIST, on_device=True, measure=True, measure_samples=5)
    calls = [c for c in net._core.engine.calls if c[0] != "set_normalise"]
    assert len(calls) == 1 and calls[0][0] == "infer_fields_measure_mc"
    # two consecutive seeds: the pass, then the Monte-Carlo decodes
    assert calls[0][1:5] == (8, 9, 5, True) and net._core.seed_counter == 9
    assert np.array_equal(calls[0][5], int((F - CS) / 2) + np.array([[0, 0], [5, -7], [-3, 11]]))
    want = np.dtype(DeblendFieldBatch.ON_DEVICE_COLUMNS + DeblendFieldBatch.measure_columns(NB) +
                    DeblendFieldBatch.measure_mc_columns(NB))
    cat, mc = stub_catalogue(3), stub_mc_catalogue(3)
    assert [len(r) for r in res] == [2, 0, 1, 0] and all(r.dtype == want for r in res)
    for i, (m, k) in enumerate([(0, 0), (0, 1), (2, 0)]):              # (field, row) of global stamps 0, 1, 2
        rec = res[m]
        assert np.array_equal(rec["flux"][k], cat["flux"][i]) and rec["Mcc"][k] == cat["shape"][i, 4]
        assert np.array_equal(rec["flux_mc_mean"][k], mc["flux_mc_mean"][i])
        assert np.array_equal(rec["flux_mc_std"][k], mc["flux_mc_std"][i]) and rec["n_ok"][k] == 3
        for q, name in enumerate(mmo.SHAPE_NAMES):
            assert rec[name + "_mc_mean"][k] == mc["shape_mc_mean"][i, q] and rec[name + "_mc_std"][k] == mc["shape_mc_std"][i, q]
    assert b.get_predicted_fields()["predicted_mean_fields"].shape == (4, F, F, NB)
    # the columns shared with the call without measure_samples are the same (the stub encodes the stamp number)
    net2, b2 = _batch()
    plain = b2.deblend_fields(DIST, on_device=True, measure=True)
    for r, p in zip(res, plain):
        for k in p.dtype.names:
            if k != "shifts":
                assert np.array_equal(r[k], p[k], equal_nan=p.dtype[k].kind == "f"), k
    # the catalogue-only form
    res2 = b.deblend_fields(DIST, on_device=True, measure=True, measure_samples=2, return_fields=False)
    call = [c for c in net._core.engine.calls if c[0] == "infer_fields_measure_mc"][-1]
    assert call[1:5] == (10, 11, 2, False) and call[5] is None
    assert all(r.dtype == want for r in res2) and np.array_equal(res2[0]["e1_mc_std"], res[0]["e1_mc_std"])
    with pytest.raises(ValueError, match="catalogue-only"):
        b.get_predicted_fields()


def test_deblend_fields_measure_samples_refusals_come_before_any_engine_call():
    net, b = _batch()
    with pytest.raises(ValueError, match="measure_samples cannot be combined"):
        b.deblend_fields(DIST, on_device=True, measure=True, measure_samples=3, optimise_positions=True)
    with pytest.raises(ValueError, match="measure_samples cannot be combined"):
        b.deblend_fields(DIST, on_device=True, measure=True, measure_samples=3, epistemic_uncertainty_estimation=True)
    with pytest.raises(ValueError, match="measure_samples needs measure=True and on_device=True"):
        b.deblend_fields(DIST, on_device=True, measure_samples=3)
    with pytest.raises(ValueError, match="measure_samples needs measure=True and on_device=True"):
        b.deblend_fields(DIST, measure=True, measure_samples=3)
    for bad in (-1, 2.5):
        with pytest.raises(ValueError, match="measure_samples must be an integer"):
            b.deblend_fields(DIST, on_device=True, measure=True, measure_samples=bad)
    # the pinned refusal of measure=True keeps its wording
    with pytest.raises(ValueError, match="position-fit or Monte-Carlo"):
        b.deblend_fields(DIST, on_device=True, measure=True, optimise_positions=True)
    assert net._core.engine.calls == [] and net._core.seed_counter == 7
