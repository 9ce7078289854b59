"""The Monte-Carlo catalogue on the GPU (dv_scene_measure_mc, dv_infer_fields_measure_mc, DeblendFieldBatch(measure_samples=S);
DESIGN.md section 7k) against the numpy restatement of tests/measure_mc_oracle.py, the fold and the pipeline stage bit for
bit.  Bounds: a per-sample measurement agrees with the oracle to the 1e-8 (px; of the trace for M) that section 7j
established; a mean over samples moves by at most that much and a standard deviation by at most twice it, and the bound
asserted is 4e-8, twice that; fluxes to rtol 1e-12 as in section 7j (non-negative terms, any summation order)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import measure_mc_oracle as mmo
from tests import measure_oracle as mo
from tests.test_gpu_measure import CS, NB, _blob_fields, _net, _planes, _windows

pytestmark = pytest.mark.gpu

MC = ("flux_mc_mean", "flux_mc_std", "shape_mc_mean", "shape_mc_std", "n_ok")
ROWS = ("sample_flux", "sample_shape", "sample_status")
CAT = ("flux", "flux_err", "shape", "iters", "status")
SPECIAL = ("all zero", "one good", "spike among good")


def _eq(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


@functools.lru_cache(maxsize=None)
def _case(cs, nb, S, band=2):
    """(names, samples float32 (S, N, cs, cs, nb), oracle results): computed once, never written to.  Ten galaxies from the
    planes of tests/test_gpu_measure.py, every sample with multiplicative noise and a one-pixel jitter, then the three special
    galaxies"""
    pick = {"gaussian": 3, "noisy gaussian": 3, "exponential": 2, "two blobs": 2}
    planes = []
    for name, p in _planes(cs, True):
        if pick.get(name, 0) > 0:
            pick[name] -= 1
            planes.append((name, p))
    assert len(planes) == 10
    rng = np.random.default_rng(31 * cs + S)
    names = [n for n, _ in planes] + list(SPECIAL)
    samples = np.zeros((S, len(names), cs, cs, nb), np.float32)
    scale = rng.uniform(0.3, 2.0, size=nb)
    scale[band] = 1.0

    def sample(p):
        q = np.roll(p, tuple(rng.integers(-1, 2, size=2)), axis=(0, 1)) * (1.0 + 0.03 * rng.normal(size=p.shape))
        return (np.maximum(q, 0.0)[:, :, None] * scale).astype(np.float32)

    for i, (_, p) in enumerate(planes):
        for q in range(S):
            samples[q, i] = sample(p)
    g = planes[0][1]
    samples[S // 2, 11] = sample(g)                          # exactly one good sample, the others zero stamps
    for q in range(S):
        samples[q, 12] = mmo.spike_stamp(cs, nb) if q == 1 else sample(g)
    ref = mmo.measure_mc(samples, band=band)
    for a in (samples,) + tuple(ref.values()):
        a.flags.writeable = False
    return names, samples, ref


def _ctx():
    from debvader_amd import engine as E

    return E.default_context()


@pytest.mark.parametrize("cs,nb,S", [(31, 3, 6), (59, 6, 3)])
def test_scene_measure_mc_against_the_oracle(cs, nb, S):
    names, samples, ref = _case(cs, nb, S)
    # the oracle alone first: the status of every sample is what the inputs were built for, and every accepted sample
    # converged within 100 iterations
    want_status = np.zeros((len(names), S), np.int32)
    want_status[10] = 3
    want_status[11] = 3
    want_status[11, S // 2] = 0
    want_status[12, 1] = 3
    for i, name in enumerate(names):
        print(f"oracle {cs}/{nb} galaxy {i:2d} {name:17s}: status {ref['sample_status'][i].tolist()}, iterations "
              f"{ref['sample_iters'][i].tolist()}, n_ok {ref['n_ok'][i]}")
    assert np.array_equal(ref["sample_status"], want_status)
    assert ref["sample_iters"][ref["sample_status"] == 0].max() <= 100
    assert ref["n_ok"].tolist() == [S] * 10 + [0, 1, S - 1]
    assert np.isnan(ref["shape_mc_mean"][10]).all() and (ref["shape_mc_std"][11] == 0).all()
    assert (ref["shape_mc_std"][:10, :2] > 1e-3).all()       # the jitter shows in the centroid

    got = _ctx().scene_measure_mc(samples, keep_samples=True)
    assert np.array_equal(got["n_ok"], ref["n_ok"]) and np.array_equal(got["sample_status"], ref["sample_status"])
    assert got["n_ok"].dtype == np.int32 and got["sample_status"].dtype == np.int32
    ok = ref["n_ok"] > 0
    tr = np.where(ok, ref["shape_mc_mean"][:, 2] + ref["shape_mc_mean"][:, 4], 1.0)[:, None]
    unit = np.concatenate([np.ones((len(names), 2)), np.repeat(tr, 3, axis=1), np.ones((len(names), 3))], axis=1)
    d_mean = np.abs(got["shape_mc_mean"] - ref["shape_mc_mean"]) / unit
    d_std = np.abs(got["shape_mc_std"] - ref["shape_mc_std"]) / unit
    rel_f = np.abs(got["flux_mc_mean"] - ref["flux_mc_mean"]) / np.abs(ref["flux_mc_mean"]).clip(1e-300)
    print(f"gpu vs oracle {cs}/{nb}: flux mean rel {rel_f.max():.2e}, shape means {d_mean[ok].max():.2e}, shape stds "
          f"{d_std[ok].max():.2e} (px, e; M in units of the trace)")
    assert np.allclose(got["flux_mc_mean"], ref["flux_mc_mean"], rtol=1e-12, atol=0.0)
    assert np.isnan(got["shape_mc_mean"][~ok]).all() and np.isnan(got["shape_mc_std"][~ok]).all()
    assert np.isfinite(got["shape_mc_mean"][ok]).all() and np.isfinite(got["shape_mc_std"][ok]).all()
    assert d_mean[ok].max() <= 4e-8
    assert d_std[ok].max() <= 4e-8
    assert (got["shape_mc_std"][11] == 0).all()


@pytest.mark.parametrize("cs,nb,S", [(31, 3, 6), (59, 6, 3)])
def test_the_fold_bit_for_bit(cs, nb, S):
    names, samples, _ = _case(cs, nb, S)
    ctx = _ctx()
    got = ctx.scene_measure_mc(samples, keep_samples=True)
    want = mmo.fold(got["sample_flux"], got["sample_shape"], got["sample_status"])
    for k in MC:
        assert _eq(got[k], want[k]), k
    for q in range(S):
        slab = ctx.scene_measure(samples[q])
        assert np.array_equal(got["sample_flux"][:, q], slab["flux"]), q
        assert np.array_equal(got["sample_shape"][:, q], slab["shape"]), q
        assert np.array_equal(got["sample_status"][:, q], slab["status"]), q


def test_invariances_bit_for_bit():
    names, samples, _ = _case(31, 3, 6)
    ctx = _ctx()
    got = ctx.scene_measure_mc(samples, keep_samples=True)
    perm = np.random.default_rng(2).permutation(len(names))
    moved = ctx.scene_measure_mc(samples[:, perm], keep_samples=True)
    for k in MC + ROWS:
        assert _eq(moved[k], got[k][perm]), k
    for i in (0, 10, 12):
        alone = ctx.scene_measure_mc(samples[:, i:i + 1], keep_samples=True)
        for k in MC + ROWS:
            assert _eq(alone[k], got[k][i:i + 1]), (i, k)
    bare = ctx.scene_measure_mc(samples)
    assert sorted(bare) == sorted(MC) and all(_eq(bare[k], got[k]) for k in MC)
    chunked = ctx.scene_measure_mc(samples, keep_samples=True, _chunk=4)      # four library calls of 4, 4, 4 and 1 galaxies
    for k in MC + ROWS:
        assert _eq(chunked[k], got[k]), k
    # other measurement parameters reach the kernel
    other = ctx.scene_measure_mc(samples, band=0, sigma0=2.0, max_iter=7)
    assert not np.array_equal(other["n_ok"], got["n_ok"])


CASES = {"A": ([30, 0, 150, 7, 40], 3), "B": ([20], 7), "C": ([7], 2)}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_pipeline_stage_has_the_bits_of_the_stamp_level_call(dtype, case, monkeypatch):
    """A: chunks cross fields, one sample per decoder pass; B: 64 // 20 = 3 samples per pass, passes of 3, 3 and 1; C: the
    tiny-call regime, whose stamps are encoded once more for the Monte-Carlo stage"""
    counts, S = CASES[case]
    net = _net(dtype)
    eng, ctx = net._core.engine, net._core.ctx
    F = 131
    fields = _blob_fields(len(counts), F, seed=11)
    starts, places, fp = _windows(F, counts, seed=5)
    seed, mc_seed = 77, 4242
    got = eng.infer_fields_measure_mc(fields, starts, fp, places=places, seed=seed, mc_seed=mc_seed, nsamples=S,
                                      keep_samples=True)
    cut = eng.infer_fields_keep(fields, starts, fp, seed=seed)["cutouts"].astype(np.float32)
    samples = np.stack([eng.infer_mc(cut, 1, mc_seed + q)[0] for q in range(S)])
    want = ctx.scene_measure_mc(samples, keep_samples=True)
    print(f"[{dtype} {case}] n_ok of the {len(starts)} galaxies over {S} samples: "
          f"{np.bincount(want['n_ok'], minlength=S + 1).tolist()}")
    for k in MC + ROWS:
        assert _eq(got[k], want[k]), k
    plain = eng.infer_fields_measure(fields, starts, fp, places=places, seed=seed)
    for k in plain:
        assert _eq(got[k], plain[k]), k
    assert sorted(got) == sorted(tuple(plain) + MC + ROWS)
    # catalogue-only, with and without the per-sample rows
    only = eng.infer_fields_measure_mc(fields, starts, fp, seed=seed, mc_seed=mc_seed, nsamples=S, return_fields=False)
    assert sorted(only) == sorted(CAT + ("mse_center",) + MC)
    for k in only:
        assert _eq(only[k], got[k]), k
    # the fields uploaded in groups
    if len(counts) > 1:
        monkeypatch.setenv("DV_FIELDS_GROUP_MB", "10")
        grouped = eng.infer_fields_measure_mc(fields, starts, fp, places=places, seed=seed, mc_seed=mc_seed, nsamples=S,
                                              keep_samples=True)
        for k in got:
            assert _eq(grouped[k], got[k]), k
        monkeypatch.setenv("DV_FIELDS_GROUP_MB", "3")
        g2 = eng.infer_fields_measure_mc(fields, starts, fp, seed=seed, mc_seed=mc_seed, nsamples=S, return_fields=False)
        for k in only:
            assert _eq(g2[k], only[k]), k
        monkeypatch.delenv("DV_FIELDS_GROUP_MB")
    else:
        one = eng.infer_cutouts_measure_mc(fields[0], starts, places=places, seed=seed, mc_seed=mc_seed, nsamples=S)
        assert "mean_field" in one and np.array_equal(one["mean_field"], got["mean_fields"][0])
        assert all(_eq(one[k], got[k]) for k in MC)
    # the existing Monte-Carlo call is where it was: the hook is off, the per-pixel statistics are taken
    if case == "B":
        eps = eng.infer_fields_mc_keep(fields, starts, fp, seed=seed, mc_seed=mc_seed, nsamples=S)["epistemic"]
        assert np.array_equal(eps, eng.infer_mc(cut, S, mc_seed)[1])


def test_pipeline_stage_with_normalise():
    net = _net("float32")
    eng, ctx = net._core.engine, net._core.ctx
    F = 131
    fields = _blob_fields(1, F, seed=11)
    starts, places, fp = _windows(F, [30], seed=5)
    eng.set_normalise(True)
    try:
        got = eng.infer_fields_measure_mc(fields, starts, fp, seed=7, mc_seed=8, nsamples=2, return_fields=False)
        cut = eng.infer_fields_keep(fields, starts, fp, seed=7)["cutouts"].astype(np.float32)
        samples = np.stack([eng.infer_mc(cut, 1, 8 + q)[0] for q in range(2)])
    finally:
        eng.set_normalise(False)
    want = ctx.scene_measure_mc(samples)
    for k in MC:
        assert _eq(got[k], want[k]), k


def test_deblend_field_batch_measure_samples():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch

    F = 131
    fields = _blob_fields(3, F, seed=21)
    rng = np.random.default_rng(4)
    dists = [rng.integers(-30, 31, size=(n, 2)).astype(np.float64) for n in (20, 0, 75)]

    def batch():
        net = _net("float32")                                    # the same weights ...
        net._core.seed_counter = 1234                            # ... and the same sequence of noise seeds
        return net, DeblendFieldBatch(net, fields, CS, NB)

    (na, a), (nb_, b) = batch(), batch()
    res = a.deblend_fields(dists, on_device=True, measure=True, measure_samples=3)
    plain = b.deblend_fields(dists, on_device=True, measure=True)
    assert na._core.seed_counter == 1236 and nb_._core.seed_counter == 1235
    want = np.dtype(DeblendFieldBatch.ON_DEVICE_COLUMNS + DeblendFieldBatch.measure_columns(NB) +
                    DeblendFieldBatch.measure_mc_columns(NB))
    for r, p in zip(res, plain):
        assert r.dtype == want and len(r) == len(p)
        for k in p.dtype.names:
            if k == "shifts":
                assert all(np.array_equal(x, y) for x, y in zip(r[k], p[k]))
            else:
                assert np.array_equal(r[k], p[k], equal_nan=p.dtype[k].kind == "f"), k
    for k, v in a.get_predicted_fields().items():
        assert np.array_equal(v, b.get_predicted_fields()[k]), k
    # the new columns against the engine call with the same two seeds
    from debvader_amd.deblend.field_deblender import batch_windows

    starts, field_ptr, _, _ = batch_windows(F, dists, CS)
    ref = na._core.engine.infer_fields_measure_mc(fields, starts, field_ptr, seed=1235, mc_seed=1236, nsamples=3,
                                                  return_fields=False)
    for m, r in enumerate(res):
        lo, hi = int(field_ptr[m]), int(field_ptr[m + 1])
        assert np.array_equal(r["flux_mc_mean"], ref["flux_mc_mean"][lo:hi]) and np.array_equal(r["n_ok"], ref["n_ok"][lo:hi])
        assert np.array_equal(r["flux_mc_std"], ref["flux_mc_std"][lo:hi])
        for q, name in enumerate(mmo.SHAPE_NAMES):
            assert np.array_equal(r[name + "_mc_mean"], ref["shape_mc_mean"][lo:hi, q], equal_nan=True), name
            assert np.array_equal(r[name + "_mc_std"], ref["shape_mc_std"][lo:hi, q], equal_nan=True), name
    # without the fields: the same catalogue
    nc, c = batch()
    cat = c.deblend_fields(dists, on_device=True, measure=True, measure_samples=3, return_fields=False)
    for r, q in zip(res, cat):
        for k in r.dtype.names:
            if k != "shifts":
                assert np.array_equal(r[k], q[k], equal_nan=r.dtype[k].kind == "f"), k


def test_refusals_come_before_any_gpu_work_and_leave_the_engine_usable():
    from debvader_amd import _lib
    from debvader_amd.engine import Engine, _dp, _fp, _ip

    DvError, lib = _lib.DvError, _lib.lib
    net = _net("float32")
    eng, ctx = net._core.engine, net._core.ctx
    F = 131
    fields = _blob_fields(1, F, seed=11)
    starts, places, fp = _windows(F, [5], seed=5, hang=False)
    kw = dict(places=places, seed=3, mc_seed=4, nsamples=2, keep_samples=True)
    good = eng.infer_fields_measure_mc(fields, starts, fp, **kw)

    def par(band=2, sigma0=3.0, tol=1e-10, max_iter=200):
        return _lib.DvMeasureParams(band, sigma0, tol, max_iter)

    n, nb, S = 5, NB, 2
    cat = [np.zeros((n, nb)), np.zeros((n, nb)), np.zeros((n, 5)), np.zeros(n, np.int32), np.zeros(n, np.int32)]
    mc = [np.zeros((n, nb)), np.zeros((n, nb)), np.zeros((n, 8)), np.zeros((n, 8)), np.zeros(n, np.int32)]
    rows = [np.zeros((n, S, nb)), np.zeros((n, S, 5)), np.zeros((n, S), np.int32)]
    ptr = lambda a: None if a is None else _ip(a) if a.dtype == np.int32 else _dp(a)
    f2, N, args = Engine._field_args(fields, starts, fp, places)
    mean_f, std_f, res_f = np.empty(f2.shape), np.empty(f2.shape), np.empty(f2.shape)

    def pipeline(p, nsamples=S, fields_out=(None, None, None), cat=cat, mc=mc, rows=(None, None, None)):
        _lib.check(lib.dv_infer_fields_measure_mc(eng._h, *args, 9, 10, nsamples, C.byref(p), *map(ptr, fields_out), None,
                                                  *map(ptr, cat), *map(ptr, mc), *map(ptr, rows)))

    x = np.zeros((S, 2, 31, 31, 3), np.float32)
    smc = [np.zeros((2, 3)), np.zeros((2, 3)), np.zeros((2, 8)), np.zeros((2, 8)), np.zeros(2, np.int32)]
    srows = [np.zeros((2, S, 3)), np.zeros((2, S, 5)), np.zeros((2, S), np.int32)]

    def stamps(p, x=x, S=S, mc=smc, rows=(None, None, None)):
        _lib.check(lib.dv_scene_measure_mc(ctx._h, _fp(x), S, x.shape[1], x.shape[2], x.shape[4], C.byref(p), *map(ptr, mc),
                                           *map(ptr, rows)))

    bad = [(par(band=nb), "band"), (par(band=-1), "band"), (par(sigma0=0.0), "sigma0"), (par(sigma0=float("nan")), "sigma0"),
           (par(tol=0.0), "tol"), (par(tol=float("inf")), "tol"), (par(max_iter=-1), "max_iter")]
    for p, msg in bad:
        with pytest.raises(DvError, match=msg):
            pipeline(p)
    for p, msg in [(par(band=3), "band")] + bad[2:]:
        with pytest.raises(DvError, match=msg):
            stamps(p)
    for call in (pipeline, stamps):
        for s in (0, -3):
            with pytest.raises(DvError, match="at least 1"):
                call(par(), **({"nsamples": s} if call is pipeline else {"S": s}))
    for k in range(5):                                           # a missing catalogue output, a missing Monte-Carlo output
        with pytest.raises(DvError, match="flux, flux_err, shape, iters and status must all be given"):
            pipeline(par(), cat=cat[:k] + [None] + cat[k + 1:])
        with pytest.raises(DvError, match="Monte-Carlo outputs .* must all be given"):
            pipeline(par(), mc=mc[:k] + [None] + mc[k + 1:])
        with pytest.raises(DvError, match="Monte-Carlo outputs .* must all be given"):
            stamps(par(), mc=smc[:k] + [None] + smc[k + 1:])
    for k in range(3):                                           # per-sample outputs given in part
        with pytest.raises(DvError, match="per-sample outputs .* go together"):
            pipeline(par(), rows=rows[:k] + [None] + rows[k + 1:])
        with pytest.raises(DvError, match="per-sample outputs .* go together"):
            stamps(par(), rows=[None] * k + [srows[k]] + [None] * (2 - k))
    with pytest.raises(DvError, match="go together"):            # result fields given in part
        pipeline(par(), fields_out=(mean_f, None, None))
    with pytest.raises(DvError, match="go together"):
        pipeline(par(), fields_out=(None, None, res_f))
    big = np.zeros((1, 1, 91, 91, 1), np.float32)
    with pytest.raises(DvError, match="LDS"):
        stamps(par(band=0), x=big, S=1)
    with pytest.raises(DvError, match="bands"):
        stamps(par(band=0), x=np.zeros((1, 1, 9, 9, 17), np.float32), S=1)
    # the engine completes correct calls afterwards
    pipeline(par(), fields_out=(mean_f, std_f, res_f), rows=rows)
    stamps(par(), rows=srows)
    again = eng.infer_fields_measure_mc(fields, starts, fp, **kw)
    for k in good:
        assert _eq(again[k], good[k]), k
    assert np.array_equal(mean_f, eng.infer_fields_composite(fields, starts, places, fp, seed=9)["mean_fields"])
