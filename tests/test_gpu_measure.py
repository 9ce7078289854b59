"""The catalogue measurement on the GPU (dv_scene_measure, dv_infer_fields_measure, DeblendFieldBatch(measure=True); DESIGN.md
section 7j) against the numpy restatement of tests/measure_oracle.py, and the pipeline stage against the stamp-level call,
bit for bit.  The bounds are those of the specification: status equal, iters equal or one apart, fluxes to rtol 1e-12 (the
terms are non-negative: any summation order is within n * eps = 4e-13), and for converged stamps the centroid to 1e-8 px and
M to 1e-8 (Mrr + Mcc) - two iterations that both stop at a step below 1e-10 with contraction <= 0.7 lie within
2 (0.7 / 0.3) 1e-10 = 5e-10 of each other, and 1e-8 is 20 times that."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import measure_oracle as mo

pytestmark = pytest.mark.gpu

ARCH = dict(input_shape=(59, 59, 6), latent_dim=32, filters=[32, 64, 128, 256], kernels=[3, 3, 3, 3])
CS, NB = 59, 6
COUNTS = [30, 0, 150, 7, 40]      # one empty field, one with more stamps than max_batch = 64: chunks cross field boundaries
CAT = ("flux", "flux_err", "shape", "iters", "status")


def _planes(cs, full):
    """Band planes (name, (cs, cs) float64): the inputs the specification lists, every one of them"""
    rng = np.random.default_rng(100 + cs)
    ctr = (cs - 1) / 2.0
    rr, cc = np.arange(cs, dtype=np.float64)[:, None], np.arange(cs, dtype=np.float64)[None, :]
    out = [("gaussian", mo.gaussian_stamp(cs, M, off)) for M, off in
           [((6.0, 2.0, 11.0), (1.3, -2.1)), ((4.0, -1.5, 5.0), (-3.2, 0.7)), ((16.0, 5.0, 9.0), (2.5, 2.5)),
            ((2.25, 0.0, 2.25), (0.5, 0.5))][:4 if full else 1]]
    for k in range(16 if full else 1):                       # relu'd Gaussians with sigma = 0.02 noise
        a, b = rng.uniform(2.0, 9.0, size=2)
        M = (a, rng.uniform(-0.6, 0.6) * np.sqrt(a * b), b)
        g = mo.gaussian_stamp(cs, M, rng.uniform(-3.0, 3.0, size=2), amp=rng.uniform(0.5, 3.0))
        out.append(("noisy gaussian", np.maximum(g + rng.normal(0.0, 0.02, size=g.shape), 0.0)))
    for off in [(0.0, 0.0), (-0.7, 1.2), (2.4, -1.9)][:3 if full else 1]:
        out.append(("exponential", np.exp(-np.hypot(rr - ctr - off[0], cc - ctr - off[1]) / 2.0)))
    for k in range(4 if full else 0):                        # two overlapping blobs
        o1, o2 = rng.uniform(-2.0, 2.0, size=2), rng.uniform(-2.0, 2.0, size=2) + (3.0, 4.0)
        out.append(("two blobs", mo.gaussian_stamp(cs, (4.0, 0.0, 4.0), o1) + 0.6 * mo.gaussian_stamp(cs, (5.0, 1.0, 3.0), o2)))
    for sr, sc in [(-1, -1), (-1, 1), (1, -1), (1, 1)][:4 if full else 1]:      # a blob 2 px from a corner
        out.append(("corner", mo.gaussian_stamp(cs, (3.0, 0.5, 4.0), (sr * (ctr - 2.0), sc * (ctr - 2.0)))))
    for k in range(4 if full else 0):
        out.append(("uniform noise", rng.uniform(size=(cs, cs))))
    out += [("constant", np.full((cs, cs), 0.37)), ("constant", np.ones((cs, cs)))][:2 if full else 0]
    spike = np.zeros((cs, cs))
    spike[cs // 2, cs // 2] = 5.0
    out += [("zero", np.zeros((cs, cs))), ("spike", spike)]
    return out


@functools.lru_cache(maxsize=None)
def _case(cs, nb, band, full):
    """(names, mean, stddev float32 (N, cs, cs, nb), oracle results, step histories): computed once, never written to"""
    planes = _planes(cs, full)
    rng = np.random.default_rng(7 * cs + nb)
    mean = np.zeros((len(planes), cs, cs, nb), np.float32)
    for i, (_, p) in enumerate(planes):
        for b in range(nb):                                  # the other bands: the plane rescaled, on a positive floor
            mean[i, :, :, b] = p if b == band else rng.uniform(0.3, 2.0) * p + rng.uniform(0.0, 0.1, size=p.shape)
    std = rng.uniform(0.01, 0.3, size=mean.shape).astype(np.float32)
    hist = []
    ref = mo.measure(mean, std, band=band, histories=hist)
    for a in (mean, std) + tuple(ref.values()):
        a.flags.writeable = False
    return [n for n, _ in planes], mean, std, ref, hist


def _ctx():
    from debvader_amd import engine as E

    return E.default_context()


@pytest.mark.parametrize("cs,nb,band,full", [(31, 3, 2, True), (31, 6, 2, True), (59, 6, 2, False)])
def test_scene_measure_against_the_oracle(cs, nb, band, full):
    names, mean, std, ref, hist = _case(cs, nb, band, full)
    assert len(names) == (39 if full else 6)
    # the oracle alone first: every converged input took at most 100 iterations and contracted by at most 0.75 at the end
    for i, name in enumerate(names):
        if ref["status"][i] == mo.CONVERGED:
            ratio = hist[i][-1] / hist[i][-2]
            print(f"oracle {cs}/{nb} stamp {i:2d} {name:15s}: {ref['iters'][i]:3d} iterations, final step ratio {ratio:.3f}")
            assert ref["iters"][i] <= 100 and ratio <= 0.75, (i, name)
        else:
            print(f"oracle {cs}/{nb} stamp {i:2d} {name:15s}: status {ref['status'][i]} at iteration {ref['iters'][i]}")
    converged = {n for n, s in zip(names, ref["status"]) if s == mo.CONVERGED}
    assert converged >= ({"gaussian", "noisy gaussian", "exponential", "two blobs"} if full else {"gaussian", "exponential"})
    assert ref["status"][names.index("zero")] == 3 and ref["iters"][names.index("zero")] == 1
    assert ref["status"][names.index("spike")] == 3 and ref["iters"][names.index("spike")] == 2

    got = _ctx().scene_measure(mean, std, band=band)
    d_it = np.abs(got["iters"].astype(int) - ref["iters"].astype(int))
    ok = ref["status"] == mo.CONVERGED
    tr = ref["shape"][:, 2] + ref["shape"][:, 4]
    d_c = np.abs(got["shape"][:, :2] - ref["shape"][:, :2]).max(axis=1)
    d_m = np.abs(got["shape"][:, 2:] - ref["shape"][:, 2:]).max(axis=1) / np.where(ok, tr, 1.0)
    rel_f = np.abs(got["flux"] - ref["flux"]) / np.abs(ref["flux"]).clip(1e-300)
    rel_e = np.abs(got["flux_err"] - ref["flux_err"]) / ref["flux_err"]
    print(f"gpu vs oracle {cs}/{nb}: status differs on {int((got['status'] != ref['status']).sum())} stamps, iters differ by "
          f"at most {d_it.max()}, flux rel {rel_f.max():.2e}, flux_err rel {rel_e.max():.2e}, centroid {d_c[ok].max():.2e} px, "
          f"M {d_m[ok].max():.2e} of the trace ({int(ok.sum())} converged of {len(ok)})")
    assert np.array_equal(got["status"], ref["status"]), list(zip(names, got["status"], ref["status"]))
    assert d_it.max() <= 1
    assert np.allclose(got["flux"], ref["flux"], rtol=1e-12, atol=0.0)
    assert np.allclose(got["flux_err"], ref["flux_err"], rtol=1e-12, atol=0.0)
    assert d_c[ok].max() <= 1e-8
    assert d_m[ok].max() <= 1e-8
    # without stddev stamps: no flux_err, the rest has the same bits; max_iter = 0 returns the initial state
    bare = _ctx().scene_measure(mean, band=band)
    assert "flux_err" not in bare and all(np.array_equal(bare[k], got[k]) for k in bare)
    init = _ctx().scene_measure(mean[:3], std[:3], band=band, sigma0=2.5, max_iter=0)
    assert (init["status"] == 2).all() and (init["iters"] == 0).all()
    assert np.array_equal(init["shape"], np.tile([(cs - 1) / 2.0, (cs - 1) / 2.0, 6.25, 0.0, 6.25], (3, 1)))
    # a stamp's result does not depend on where it sits in the batch
    perm = np.random.default_rng(1).permutation(len(names))
    shuffled = _ctx().scene_measure(mean[perm], std[perm], band=band)
    assert all(np.array_equal(shuffled[k], got[k][perm]) for k in got)


def test_only_the_chosen_band_decides_the_shape():
    names, mean, std, ref, _ = _case(31, 6, 2, True)
    got = _ctx().scene_measure(mean, std, band=2)
    other = np.array(mean)
    other[..., [0, 1, 3, 4, 5]] = np.random.default_rng(3).uniform(size=other[..., :5].shape).astype(np.float32)
    o = _ctx().scene_measure(other, std, band=2)
    for k in ("shape", "iters", "status"):
        assert np.array_equal(o[k], got[k]), k
    assert np.array_equal(o["flux"][:, 2], got["flux"][:, 2]) and not np.array_equal(o["flux"][:, 0], got["flux"][:, 0])
    b4 = _ctx().scene_measure(other, std, band=4)
    assert not np.array_equal(b4["shape"], got["shape"])
    assert np.array_equal(b4["flux"], o["flux"]) and np.array_equal(b4["flux_err"], o["flux_err"])
    want = mo.measure(other[:6], None, band=4)
    conv = want["status"] == mo.CONVERGED
    assert np.array_equal(b4["status"][:6], want["status"]) and conv.any()
    assert np.abs(b4["shape"][:6][conv] - want["shape"][conv]).max() < 1e-6


def _blob_fields(M, F, seed, nblob=12, amp=(2.0, 9.0), noise=0.05):
    """M fields (M, F, F, 6): Gaussian blobs of random size and flux on Gaussian noise."""
    rng = np.random.default_rng(seed)
    out = rng.normal(0, noise, size=(M, F, F, NB))
    yy, xx = np.mgrid[:F, :F]
    for m in range(M):
        for _ in range(nblob):
            r, c = rng.uniform(35, F - 35, size=2)
            sig, a = rng.uniform(1.5, 3.5), rng.uniform(*amp)
            g = a * np.exp(-0.5 * ((yy - r) ** 2 + (xx - c) ** 2) / sig ** 2)
            out[m] += g[:, :, None] * rng.uniform(0.5, 1.0, size=NB)
    return out


def _net(dtype, max_batch=64, seed=3):
    from debvader_amd.model import model

    net, _, _, _ = model.create_model_vae(**ARCH, max_batch=max_batch, seed=seed, dtype=dtype)
    return net


def _windows(F, counts, seed, hang=True):
    rng = np.random.default_rng(seed)
    n = int(np.sum(counts))
    starts = rng.integers(0, F - CS + 1, size=(n, 2)).astype(np.int32)
    places = starts.copy()
    if hang:
        k = rng.random(n) < 0.3
        places[k] = rng.integers(-CS + 3, F - 3, size=(int(k.sum()), 2))
    fp = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return starts, places, fp


@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_pipeline_stage_has_the_bits_of_the_stamp_level_call(dtype, monkeypatch):
    net = _net(dtype)
    eng, ctx = net._core.engine, net._core.ctx
    F = 131
    fields = _blob_fields(5, F, seed=11)
    starts, places, fp = _windows(F, COUNTS, seed=5)
    seed = 77
    stamps = eng.infer_fields(fields, starts, fp, seed=seed)
    want = ctx.scene_measure(stamps["loc"], stamps["scale"])
    comp = eng.infer_fields_composite(fields, starts, places, fp, seed=seed)
    print(f"[{dtype}] status of the {len(starts)} network stamps: {np.bincount(want['status'], minlength=4).tolist()}, "
          f"iterations {want['iters'].min()} .. {want['iters'].max()}")

    got = eng.infer_fields_measure(fields, starts, fp, places=places, seed=seed)
    for k in CAT:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    for k in comp:
        assert np.array_equal(got[k], comp[k]), k
    assert sorted(got) == sorted(CAT + tuple(comp))
    # the catalogue-only call
    only = eng.infer_fields_measure(fields, starts, fp, seed=seed, return_fields=False)
    assert sorted(only) == sorted(CAT + ("mse_center",))
    for k in only:
        assert np.array_equal(only[k], got[k]), k
    bare = eng.infer_fields_measure(fields, starts, fp, seed=seed, return_fields=False, mse_center=False)
    assert sorted(bare) == sorted(CAT) and all(np.array_equal(bare[k], want[k]) for k in CAT)
    # the fields uploaded in groups of three (see tests/test_gpu_fields_batch.py), with and without result fields
    monkeypatch.setenv("DV_FIELDS_GROUP_MB", "10")
    grouped = eng.infer_fields_measure(fields, starts, fp, places=places, seed=seed)
    for k in got:
        assert np.array_equal(grouped[k], got[k]), k
    monkeypatch.setenv("DV_FIELDS_GROUP_MB", "3")
    g2 = eng.infer_fields_measure(fields, starts, fp, seed=seed, return_fields=False)
    for k in only:
        assert np.array_equal(g2[k], only[k]), k
    monkeypatch.delenv("DV_FIELDS_GROUP_MB")
    # other measurement parameters reach the kernel
    b0 = eng.infer_fields_measure(fields, starts, fp, seed=seed, return_fields=False, band=0, sigma0=2.0, max_iter=7)
    w0 = ctx.scene_measure(stamps["loc"], stamps["scale"], band=0, sigma0=2.0, max_iter=7)
    assert all(np.array_equal(b0[k], w0[k]) for k in CAT) and not np.array_equal(w0["shape"], want["shape"])
    # normalise=True: the denormalised stamps the composite stage adds are the ones measured
    eng.set_normalise(True)
    try:
        sn = eng.infer_fields(fields[:1], starts[:30], fp[:2], seed=seed)
        mn = eng.infer_fields_measure(fields[:1], starts[:30], fp[:2], seed=seed, return_fields=False)
    finally:
        eng.set_normalise(False)
    wn = ctx.scene_measure(sn["loc"], sn["scale"])
    assert all(np.array_equal(mn[k], wn[k]) for k in CAT) and not np.array_equal(wn["flux"], want["flux"][:30])
    # M = 1 is the single-field view
    s1, p1, fp1 = _windows(F, [150], seed=9)
    one = eng.infer_fields_measure(fields[2:3], s1, fp1, places=p1, seed=seed)
    ref = eng.infer_cutouts_measure(fields[2], s1, places=p1, seed=seed)
    assert "mean_field" in ref and np.array_equal(one["mean_fields"][0], ref["mean_field"])
    assert np.array_equal(one["residual_fields"][0], ref["residual_field"])
    for k in CAT + ("mse_center",):
        assert np.array_equal(one[k], ref[k]), k


def test_deblend_field_batch_measures_on_the_device():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch

    F = 131
    fields = _blob_fields(3, F, seed=21)
    rng = np.random.default_rng(4)
    dists = [rng.integers(-30, 31, size=(n, 2)).astype(np.float64) for n in (20, 0, 75)]
    def batch():
        net = _net("float32")                                    # the same weights ...
        net._core.seed_counter = 1234                            # ... and the same sequence of noise seeds (random per net)
        return DeblendFieldBatch(net, fields, CS, NB)

    a, b = batch(), batch()
    res = a.deblend_fields(dists, on_device=True, measure=True)
    plain = b.deblend_fields(dists, on_device=True)
    want = np.dtype(DeblendFieldBatch.ON_DEVICE_COLUMNS + DeblendFieldBatch.measure_columns(NB))
    for m, (r, p) in enumerate(zip(res, plain)):
        assert r.dtype == want and p.dtype == np.dtype(DeblendFieldBatch.ON_DEVICE_COLUMNS)
        assert len(r) == len(dists[m]) == len(p)
        for k in p.dtype.names:                                   # today's columns, value for value
            if k == "shifts":
                assert all(np.array_equal(x, y) for x, y in zip(r[k], p[k]))
            else:
                assert np.array_equal(r[k], p[k]), k
        start = -int(CS / 2) + dists[m] + int(F / 2)
        assert np.array_equal(r["measured_distance_x"], start[:, 0] + r["row"] - int(F / 2))
        assert np.array_equal(r["measured_distance_y"], start[:, 1] + r["col"] - int(F / 2))
        assert r["flux"].shape == (len(r), NB) and np.isfinite(r["flux"]).all() and (r["flux_err"] > 0).all()
        ok = r["status"] == 0
        assert np.isnan(r["sigma"][r["status"] == 3]).all()
        assert np.array_equal(r["sigma"][ok], np.sqrt(np.sqrt(r["Mrr"] * r["Mcc"] - r["Mrc"] ** 2))[ok])
    for k, v in a.get_predicted_fields().items():
        assert np.array_equal(v, b.get_predicted_fields()[k]), k
    assert np.array_equal(a.get_residual_fields(), b.get_residual_fields())
    # the catalogue-only pass of a third, identical object: the same catalogue, no fields
    c = batch()
    cat = c.deblend_fields(dists, on_device=True, measure=True, return_fields=False)
    for r, q in zip(res, cat):
        for k in r.dtype.names:
            if k != "shifts":
                assert np.array_equal(r[k], q[k], equal_nan=r.dtype[k].kind == "f"), k
    with pytest.raises(ValueError, match="catalogue-only"):
        c.get_predicted_fields()


def test_refusals_come_before_any_gpu_work_and_leave_the_engine_usable():
    from debvader_amd import _lib
    from debvader_amd.engine import Engine, _dp, _fp, _ip

    DvError, lib = _lib.DvError, _lib.lib
    net = _net("float32")
    eng, ctx = net._core.engine, net._core.ctx
    F = 131
    fields = _blob_fields(1, F, seed=11)
    starts, places, fp = _windows(F, [5], seed=5, hang=False)
    good = eng.infer_fields_measure(fields, starts, fp, places=places, seed=3)

    def par(band=2, sigma0=3.0, tol=1e-10, max_iter=200):
        return _lib.DvMeasureParams(band, sigma0, tol, max_iter)

    n, nb = 5, NB
    flux, ferr, shape = np.zeros((n, nb)), np.zeros((n, nb)), np.zeros((n, 5))
    iters, status = np.zeros(n, np.int32), np.zeros(n, np.int32)
    f2, N, args = Engine._field_args(fields, starts, fp, places)
    mean_f, std_f, res_f = np.empty(f2.shape), np.empty(f2.shape), np.empty(f2.shape)

    def pipeline(p, fields_out=(None, None, None), cat=None):
        cat = cat or (_dp(flux), _dp(ferr), _dp(shape), _ip(iters), _ip(status))
        _lib.check(lib.dv_infer_fields_measure(eng._h, *args, 9, C.byref(p), *fields_out, None, *cat))

    mean = np.zeros((2, 31, 31, 3), np.float32)
    held = [np.zeros((2, 3)), np.zeros((2, 3)), np.zeros((2, 5)), np.zeros(2, np.int32), np.zeros(2, np.int32)]
    out = (_dp(held[0]), _dp(held[1]), _dp(held[2]), _ip(held[3]), _ip(held[4]))

    def stamps(p, x=mean, sd=mean, o=out):
        _lib.check(lib.dv_scene_measure(ctx._h, _fp(x), _fp(sd), x.shape[0], x.shape[1], x.shape[3], C.byref(p), *o))

    bad = [(par(band=nb), "band"), (par(band=-1), "band"), (par(sigma0=0.0), "sigma0"), (par(sigma0=float("nan")), "sigma0"),
           (par(tol=0.0), "tol"), (par(tol=float("inf")), "tol"), (par(max_iter=-1), "max_iter")]
    for p, msg in bad:
        with pytest.raises(DvError, match=msg):
            pipeline(p)
    for p, msg in [(par(band=3), "band")] + bad[2:]:
        with pytest.raises(DvError, match=msg):
            stamps(p)
    # a missing catalogue output, half a set of fields, stddev without flux_err, a stamp whose plane does not fit the LDS
    for k in range(5):
        cat = [_dp(flux), _dp(ferr), _dp(shape), _ip(iters), _ip(status)]
        cat[k] = None
        with pytest.raises(DvError, match="must all be given"):
            pipeline(par(), cat=tuple(cat))
    with pytest.raises(DvError, match="go together"):
        pipeline(par(), fields_out=(_dp(mean_f), None, None))
    with pytest.raises(DvError, match="go together"):
        pipeline(par(), fields_out=(None, None, _dp(res_f)))
    with pytest.raises(DvError, match="must all be given"):
        stamps(par(), o=(out[0], out[1], None, out[3], out[4]))
    with pytest.raises(DvError, match="go together"):
        stamps(par(), o=(out[0], None) + out[2:])
    big = np.zeros((1, 91, 91, 1), np.float32)
    with pytest.raises(DvError, match="LDS"):
        stamps(par(band=0), x=big, sd=big)
    with pytest.raises(DvError, match="bands"):
        stamps(par(band=0), x=np.zeros((1, 9, 9, 17), np.float32), sd=np.zeros((1, 9, 9, 17), np.float32))
    # cs = 90 is the largest stamp the kernel takes
    edge = np.random.default_rng(0).uniform(size=(2, 90, 90, 1)).astype(np.float32)
    e = ctx.scene_measure(edge, edge, band=0)
    w = mo.measure(edge, edge, band=0)
    assert np.array_equal(e["status"], w["status"]) and np.allclose(e["flux"], w["flux"], rtol=1e-12)
    # the engine completes a correct call afterwards
    pipeline(par(), fields_out=(_dp(mean_f), _dp(std_f), _dp(res_f)))
    again = eng.infer_fields_measure(fields, starts, fp, places=places, seed=3)
    for k in good:
        assert np.array_equal(again[k], good[k]), k
    assert np.array_equal(mean_f, eng.infer_fields_composite(fields, starts, places, fp, seed=9)["mean_fields"])
