"""The Monte-Carlo epistemic estimate as a stage of the many-field engine calls (dv_infer_fields_mc_keep, _mc_composite; DESIGN.md
section 7g) against the entry points it fuses: dv_infer_fields_keep / _composite for the deblending pass, dv_infer_mc for
the std stamps, dv_scene_composite for the epistemic fields.  Every comparison is bit for bit except eps_norm, whose sums
the kernel adds in an order of its own (see test_eps_norm).  Small inputs, as in tests/test_gpu_fields_batch.py."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ARCH = dict(input_shape=(59, 59, 6), latent_dim=32, filters=[32, 64, 128, 256], kernels=[3, 3, 3, 3])
CS, NB = 59, 6
F = 160
COUNTS = [30, 0, 150, 7, 40]      # one empty field, one with more stamps than max_batch = 64: chunks cross field boundaries
SEED, MC_SEED, NS = 77, 1234, 8


def _blob_fields(M, F, seed, nblob=12, amp=(2.0, 9.0), noise=0.05):
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


def _case(F, counts, seed, hang=True):
    rng = np.random.default_rng(seed)
    n = int(np.sum(counts))
    starts = rng.integers(0, F - CS + 1, size=(n, 2)).astype(np.int32)
    places = starts.copy()
    if hang:
        k = rng.random(n) < 0.3
        places[k] = rng.integers(-CS + 3, F - 3, size=(int(k.sum()), 2))
    fp = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return starts, places, fp


def _epistemic_fields(net, eps, places, fp, shape):
    """ctx.scene_composite of the std stamps (as float64) per field, in object order"""
    ctx = net._core.ctx
    po = int((shape[1] - CS) / 2)
    out, zeros = np.zeros(shape), np.zeros(shape[1:])
    for m in range(shape[0]):
        lo, hi = int(fp[m]), int(fp[m + 1])
        if hi > lo:
            out[m] = ctx.scene_composite(zeros, eps[lo:hi].astype(np.float64), (places[lo:hi] - po).astype(np.float64))
    return out


@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_engine_calls_equal_the_calls_they_fuse(dtype, monkeypatch):
    net = _net(dtype)
    eng = net._core.engine
    fields = _blob_fields(5, F, seed=11)
    starts, places, fp = _case(F, COUNTS, seed=5)
    assert (places < 0).any() and (places > F - CS).any()          # stamps hang over the edges

    # 1. keep form: the deblending pass is infer_fields_keep's, the std stamps are infer_mc's on the float32 cutouts
    keep = eng.infer_fields_keep(fields, starts, fp, seed=SEED)
    mck = eng.infer_fields_mc_keep(fields, starts, fp, seed=SEED, mc_seed=MC_SEED, nsamples=NS)
    assert sorted(mck) == ["cutouts", "epistemic", "loc", "scale"]
    for k in ("loc", "scale", "cutouts"):
        assert mck[k].dtype == keep[k].dtype and np.array_equal(mck[k], keep[k]), k
    eps = eng.infer_mc(keep["cutouts"].astype(np.float32), NS, seed=MC_SEED)[1]
    assert mck["epistemic"].dtype == np.float32 and mck["epistemic"].shape == eps.shape
    ndiff = int((mck["epistemic"] != eps).sum())
    print(f"[{dtype}] epistemic stamps vs infer_mc: {ndiff} of {eps.size} elements differ, "
          f"max abs difference {np.abs(mck['epistemic'] - eps).max():.3e}")
    assert np.array_equal(mck["epistemic"], eps)
    assert eps.max() > 0 and np.isfinite(eps).all()
    other_seed = eng.infer_fields_mc_keep(fields, starts, fp, seed=SEED, mc_seed=MC_SEED + 1, nsamples=NS)
    assert np.array_equal(other_seed["loc"], keep["loc"]) and not np.array_equal(other_seed["epistemic"], eps)

    # 2. composite form: mean / stddev / residual / mse_center are infer_fields_composite's, the epistemic fields are
    # dv_scene_composite of the std stamps in object order
    comp = eng.infer_fields_composite(fields, starts, places, fp, seed=SEED)
    mcc = eng.infer_fields_mc_composite(fields, starts, places, fp, seed=SEED, mc_seed=MC_SEED, nsamples=NS)
    assert set(mcc) == {"eps_norm", "epistemic_fields", "mean_fields", "mse_center", "residual_fields", "stddev_fields"}
    for k in comp:
        assert np.array_equal(mcc[k], comp[k]), k
    want_f = _epistemic_fields(net, eps, places, fp, fields.shape)
    assert np.array_equal(mcc["epistemic_fields"], want_f)
    assert not mcc["epistemic_fields"][1].any() and np.abs(want_f[0]).max() > 0
    part = eng.infer_fields_mc_composite(fields, starts, places, fp, seed=SEED, mc_seed=MC_SEED, nsamples=NS, residual=False,
                                         mse_center=False)
    assert set(part) == {"eps_norm", "epistemic_fields", "mean_fields", "stddev_fields"}
    assert np.array_equal(part["epistemic_fields"], want_f) and np.array_equal(part["eps_norm"], mcc["eps_norm"])

    # 3. fields uploaded in groups of three (five 1.2-MB buffers per field with the estimate on: 19 MB hold three): chunks
    # 0-2 run with fields 0-2 resident, chunk 3 with fields 2-4, and field 2's three sums travel from one group to the next
    monkeypatch.setenv("DV_FIELDS_GROUP_MB", "19")
    grouped = eng.infer_fields_mc_composite(fields, starts, places, fp, seed=SEED, mc_seed=MC_SEED, nsamples=NS)
    for k in mcc:
        assert np.array_equal(grouped[k], mcc[k]), k
    monkeypatch.setenv("DV_FIELDS_GROUP_MB", "4")          # three 1.2-MB fields at a time
    g2 = eng.infer_fields_mc_keep(fields, starts, fp, seed=SEED, mc_seed=MC_SEED, nsamples=NS)
    for k in mck:
        assert np.array_equal(g2[k], mck[k]), k
    # the existing call's groups are sized as before (four buffers per field): 15 MB hold three of its fields, not three
    # fields of the call with the estimate
    from debvader_amd._lib import DvError
    monkeypatch.setenv("DV_FIELDS_GROUP_MB", "15")
    assert np.array_equal(eng.infer_fields_composite(fields, starts, places, fp, seed=SEED)["mean_fields"], comp["mean_fields"])
    with pytest.raises(DvError, match="lower max_batch"):
        eng.infer_fields_mc_composite(fields, starts, places, fp, seed=SEED, mc_seed=MC_SEED, nsamples=NS)
    monkeypatch.setenv("DV_FIELDS_GROUP_MB", "5")           # one field with the estimate needs 6.1 MB
    with pytest.raises(DvError, match="needs"):
        eng.infer_fields_mc_composite(fields, starts, places, fp, seed=SEED, mc_seed=MC_SEED, nsamples=NS)
    monkeypatch.delenv("DV_FIELDS_GROUP_MB")

    # 4. M = 1 against the single-field wrappers; the rows are stamps 0 .. 149 of a list of their own
    s1, p1, fp1 = _case(F, [150], seed=9)
    one = eng.infer_fields_mc_composite(fields[2:3], s1, p1, fp1, seed=SEED, mc_seed=MC_SEED, nsamples=NS)
    ref = eng.infer_cutouts_mc_composite(fields[2], s1, p1, seed=SEED, mc_seed=MC_SEED, nsamples=NS)
    assert set(ref) == {"eps_norm", "epistemic_field", "mean_field", "mse_center", "residual_field", "stddev_field"}
    for k in ("mean", "stddev", "epistemic", "residual"):
        assert np.array_equal(one[k + "_fields"][0], ref[k + "_field"]), k
    assert np.array_equal(one["eps_norm"], ref["eps_norm"]) and np.array_equal(one["mse_center"], ref["mse_center"])
    plain = eng.infer_cutouts_composite(fields[2], s1, p1, seed=SEED)
    assert np.array_equal(ref["mean_field"], plain["mean_field"]) and np.array_equal(ref["mse_center"], plain["mse_center"])
    k1 = eng.infer_cutouts_mc_keep(fields[2], s1, seed=SEED, mc_seed=MC_SEED, nsamples=NS)
    e1 = eng.infer_mc(k1["cutouts"].astype(np.float32), NS, seed=MC_SEED)[1]
    assert np.array_equal(k1["epistemic"], e1)
    assert np.array_equal(ref["epistemic_field"], _epistemic_fields(net, e1, p1, fp1, fields[2:3].shape)[0])
    # a call of at most 16 stamps (the small-call kernels run its deblending pass): still infer_mc's bits
    k7 = eng.infer_cutouts_mc_keep(fields[3], s1[:7], seed=SEED, mc_seed=MC_SEED, nsamples=NS)
    p7 = eng.infer_cutouts_keep(fields[3], s1[:7], seed=SEED)
    assert np.array_equal(k7["loc"], p7["loc"]) and np.array_equal(k7["scale"], p7["scale"])
    assert np.array_equal(k7["epistemic"], eng.infer_mc(k7["cutouts"].astype(np.float32), NS, seed=MC_SEED)[1])

    # 5. a second run gives the same bits, and a field's results do not depend on the other fields' pixels
    again = eng.infer_fields_mc_composite(fields, starts, places, fp, seed=SEED, mc_seed=MC_SEED, nsamples=NS)
    for k in mcc:
        assert np.array_equal(again[k], mcc[k]), k
    other = _blob_fields(5, F, seed=12)
    other[2] = fields[2]
    o2 = eng.infer_fields_mc_composite(other, starts, places, fp, seed=SEED, mc_seed=MC_SEED, nsamples=NS)
    for k in ("mean_fields", "stddev_fields", "epistemic_fields", "residual_fields"):
        assert np.array_equal(o2[k][2], mcc[k][2]), k
        assert not np.array_equal(o2[k][0], mcc[k][0]), k
    assert np.array_equal(o2["eps_norm"][fp[2]:fp[3]], mcc["eps_norm"][fp[2]:fp[3]])

    # 6. normalise=True: the statistics of the denormalised means, as infer_mc folds them
    eng.set_normalise(True)
    try:
        kn = eng.infer_fields_mc_keep(fields[:1], starts[:30], fp[:2], seed=SEED, mc_seed=MC_SEED, nsamples=NS)
        pn = eng.infer_fields_keep(fields[:1], starts[:30], fp[:2], seed=SEED)
        en = eng.infer_mc(kn["cutouts"].astype(np.float32), NS, seed=MC_SEED)[1]
    finally:
        eng.set_normalise(False)
    assert np.array_equal(kn["loc"], pn["loc"]) and np.array_equal(kn["epistemic"], en)
    assert not np.array_equal(en, eps[:30])


@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_chunks_and_samples_per_pass_that_differ_from_infer_mc(dtype):
    """max_batch 256 and 150 stamps: the pipeline cuts 128 + 22 stamps and decodes 2 and 11 samples per pass (the
    multi-sample Welford fold), infer_mc takes the 150 stamps as one chunk with one sample per pass.  Same bits: the noise
    of (stamp, sample), the fold order and the decoder's rows do not depend on either split."""
    net = _net(dtype, max_batch=256)
    eng = net._core.engine
    fields = _blob_fields(1, F, seed=11)
    s1, p1, fp1 = _case(F, [150], seed=9)
    keep = eng.infer_fields_keep(fields, s1, fp1, seed=SEED)
    mck = eng.infer_fields_mc_keep(fields, s1, fp1, seed=SEED, mc_seed=MC_SEED, nsamples=NS)
    assert np.array_equal(mck["loc"], keep["loc"]) and np.array_equal(mck["scale"], keep["scale"])
    eps = eng.infer_mc(keep["cutouts"].astype(np.float32), NS, seed=MC_SEED)[1]
    print(f"[{dtype}] 128 + 22 against 150: {int((mck['epistemic'] != eps).sum())} of {eps.size} elements differ")
    assert np.array_equal(mck["epistemic"], eps) and eps.max() > 0
    mcc = eng.infer_fields_mc_composite(fields, s1, p1, fp1, seed=SEED, mc_seed=MC_SEED, nsamples=NS)
    assert np.array_equal(mcc["epistemic_fields"], _epistemic_fields(net, eps, p1, fp1, fields.shape))


@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_eps_norm(dtype):
    """eps_norm[i] = sum(std[i, :, :, 2]) / sum(mean[i, :, :, 2]), both sums in float64 on the GPU.

    Against the same formula in float64 on the returned stamps only the order of the 3481 additions differs: rtol 1e-12
    (3481 * 2^-53 = 4e-13 bounds the reordering error of a sum of non-negative terms).  Against DeblendField's host value
    the denominator is numpy's float32 pairwise sum of the float32 means, which are relu outputs >= 0: its relative error
    is at most about log2(3481) * 2^-24 = 7e-7, so rtol 2e-6.  normalise=False."""
    net = _net(dtype)
    eng = net._core.engine
    fields = _blob_fields(5, F, seed=11)
    starts, places, fp = _case(F, COUNTS, seed=5)
    mck = eng.infer_fields_mc_keep(fields, starts, fp, seed=SEED, mc_seed=MC_SEED, nsamples=NS)
    mcc = eng.infer_fields_mc_composite(fields, starts, places, fp, seed=SEED, mc_seed=MC_SEED, nsamples=NS)
    e64, m64 = mck["epistemic"].astype(np.float64), mck["loc"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        exact = e64[:, :, :, 2].sum(axis=(1, 2)) / m64[:, :, :, 2].sum(axis=(1, 2))
        host = np.array([np.sum(e[:, :, 2]) for e in e64]) / np.array([np.sum(m[:, :, 2]) for m in mck["loc"]])
    got = mcc["eps_norm"]
    assert got.dtype == np.float64 and got.shape == (int(fp[-1]),)
    fin = np.isfinite(exact)
    print(f"[{dtype}] eps_norm: {int(fin.sum())} of {len(fin)} finite, range {np.nanmin(exact):.3e} .. {np.nanmax(exact):.3e}, "
          f"max rel to the float64 formula {np.max(np.abs(got[fin] - exact[fin]) / exact[fin]):.3e}, "
          f"to the host formula {np.max(np.abs(got[fin] - host[fin]) / host[fin]):.3e}")
    assert fin.sum() >= len(fin) // 2                                    # the comparison is not vacuous
    assert np.array_equal(np.isnan(got), np.isnan(exact)) and np.array_equal(np.isinf(got), np.isinf(exact))
    np.testing.assert_allclose(got[fin], exact[fin], rtol=1e-12, atol=0)
    np.testing.assert_allclose(got[fin], host[fin], rtol=2e-6, atol=0)


@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_classes_give_the_same_results_in_both_modes(dtype):
    from debvader_amd.deblend.field_deblender import DeblendField, DeblendFieldBatch
    from debvader_amd.deblend_cutout.deblender import deblend_epistemic

    net = _net(dtype)
    eng, core = net._core.engine, net._core
    fields = _blob_fields(5, F, seed=31, nblob=9)
    rng = np.random.default_rng(4)
    half = (F - CS) // 2
    dist = [np.round(rng.uniform(-half + 1, half - 1, size=(n, 2))) for n in (30, 0, 150, 7, 40)]
    dist[3] = np.concatenate([dist[3], [[half + 30.0, 0.0]]])           # one galaxy of field 3 leaves the field

    # DeblendField, estimate on (100 samples): default and on-device mode from the same seed_counter
    m = 3
    a = DeblendField(net, fields[m:m + 1], epistemic_uncertainty_estimation=True)
    core.seed_counter = 300
    ra = a.deblend_field(dist[m], mse_criterion=1e9)
    assert core.seed_counter == 302                                      # deblending pass, then Monte Carlo
    pa = a.get_predicted_field()
    b = DeblendField(net, fields[m:m + 1], epistemic_uncertainty_estimation=True)
    core.seed_counter = 300
    rb = b.deblend_field(dist[m], mse_criterion=1e9, on_device=True)
    assert core.seed_counter == 302
    pb = b.get_predicted_field()
    assert len(ra) == 7 and len(rb) == 7 and "epistemic_norm" in rb.dtype.names
    for k in ("predicted_mean_field", "predicted_stddev_field", "predicted_epistemic_field"):
        assert np.array_equal(pa[k], pb[k]), k
    assert np.abs(pa["predicted_epistemic_field"]).max() > 0
    assert list(ra["passed_cuts"]) == list(rb["passed_cuts"])
    assert np.array_equal(a.get_residual_field(), b.get_residual_field())
    # the default path's recarray is what the two calls it replaced give: infer_cutouts_keep, then deblend_epistemic
    from debvader_amd.extract.extraction import cutout_windows
    st, ok = cutout_windows(F, dist[m], CS)
    core.seed_counter = 300
    old = eng.infer_cutouts_keep(fields[m], st[ok], seed=core.next_seed())
    _, old_eps = deblend_epistemic(net, old["cutouts"], n_samples=100)
    for i in range(7):
        assert np.array_equal(ra["output_images_mean"][i], old["loc"][i])
        assert np.array_equal(ra["output_images_stddev"][i], old["scale"][i])
        assert np.array_equal(ra["cutout_images"][i], old["cutouts"][i])
        assert np.array_equal(ra["epistemic_uncertainty"][i], old_eps[i].astype(np.float64))
    host_norm = np.array([np.sum(e[:, :, 2]) for e in ra["epistemic_uncertainty"]]) / \
        np.array([np.sum(x[:, :, 2]) for x in ra["output_images_mean"]])
    np.testing.assert_allclose(rb["epistemic_norm"], host_norm, rtol=2e-6, atol=0)

    # DeblendFieldBatch, estimate on with 8 samples: both modes, and the engine-level expectations per field
    da = DeblendFieldBatch(net, fields)
    core.seed_counter = 500
    res_a = da.deblend_fields(dist, mse_criterion=1e9, epistemic_uncertainty_estimation=True, epistemic_samples=NS)
    assert core.seed_counter == 502
    fa = da.get_predicted_fields()
    dbb = DeblendFieldBatch(net, fields)
    core.seed_counter = 500
    res_b = dbb.deblend_fields(dist, mse_criterion=1e9, on_device=True, epistemic_uncertainty_estimation=True,
                               epistemic_samples=NS)
    fb = dbb.get_predicted_fields()
    assert sorted(fa) == sorted(fb) == ["predicted_epistemic_fields", "predicted_mean_fields", "predicted_stddev_fields"]
    for k in fa:
        assert np.array_equal(fa[k], fb[k]), k
    assert np.array_equal(da.get_residual_fields(), dbb.get_residual_fields())
    assert [len(r) for r in res_a] == [30, 0, 150, 7, 40] and [len(r) for r in res_b] == [30, 0, 150, 7, 40]
    for x, y in zip(res_a, res_b):
        assert list(x["passed_cuts"]) == list(y["passed_cuts"])
    from debvader_amd.deblend.field_deblender import batch_windows
    starts, fp, kept, dd = batch_windows(F, dist, CS)
    places = (int((F - CS) / 2) + dd).astype(np.int64)
    exp = eng.infer_fields_mc_keep(fields, starts, fp, seed=501, mc_seed=502, nsamples=NS)
    for mm in range(5):
        lo = int(fp[mm])
        for i in range(len(res_a[mm])):
            assert np.array_equal(res_a[mm]["output_images_mean"][i], exp["loc"][lo + i])
            assert res_a[mm]["epistemic_uncertainty"][i].dtype == np.float64
            assert np.array_equal(res_a[mm]["epistemic_uncertainty"][i], exp["epistemic"][lo + i].astype(np.float64))
    assert np.array_equal(fb["predicted_epistemic_fields"], _epistemic_fields(net, exp["epistemic"], places, fp, fields.shape))
    # a pass without the estimate after one with it: today's keys and zeros
    core.seed_counter = 500
    dbb.deblend_fields(dist, on_device=True)
    assert sorted(dbb.get_predicted_fields()) == ["predicted_mean_fields", "predicted_stddev_fields"]

    # a criterion between two measured eps_norm values cuts exactly the galaxies above it (the widest gap between two
    # neighbouring values, so that the host formula's 2e-6 cannot move a galaxy across it)
    norm = np.concatenate([r["epistemic_norm"] for r in res_b])
    srt = np.sort(norm[np.isfinite(norm)])
    gaps = np.diff(srt)
    j = int(np.argmax(gaps[len(srt) // 4: 3 * len(srt) // 4])) + len(srt) // 4
    crit = 0.5 * (srt[j] + srt[j + 1])
    assert gaps[j] > 1e-4 * crit
    for on_device, d in ((True, dbb), (False, da)):
        core.seed_counter = 500
        res = d.deblend_fields(dist, mse_criterion=1e9, on_device=on_device, epistemic_uncertainty_estimation=True,
                               epistemic_criterion=crit, epistemic_samples=NS)
        passed = np.concatenate([r["passed_cuts"] for r in res])
        assert np.array_equal(passed, ~(norm > crit))
        assert 0 < passed.sum() < len(passed)


def test_refusals_leave_the_engine_usable():
    from debvader_amd import _lib
    from debvader_amd._lib import DvError
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch

    net = _net("float32")
    eng = net._core.engine
    fields = _blob_fields(2, F, seed=41)
    starts, places, fp = _case(F, [5, 3], seed=2)
    with pytest.raises(ValueError, match="nsamples"):
        eng.infer_fields_mc_keep(fields, starts, fp, nsamples=0)
    with pytest.raises(ValueError, match="band 2"):
        eng.infer_fields_mc_composite(fields[..., :2], starts, places, fp)
    # the library's own refusals, reached past the Python checks: no samples, two bands, a missing output
    n = len(starts)
    dp, fpp, ip = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32)
    loc = np.zeros((n, CS, CS, NB), np.float32)
    cut = np.zeros((n, CS, CS, NB), np.float64)
    fl = np.zeros(fields.shape)
    en = np.zeros(n)
    pl = np.ascontiguousarray(places, dtype=np.int32)
    keep_args = lambda nb, ns, eps: (eng._h, fields.ctypes.data_as(dp), 2, F, nb, starts.ctypes.data_as(ip),
                                     fp.ctypes.data_as(C.POINTER(C.c_int64)), n, 1, 2, ns, loc.ctypes.data_as(fpp),
                                     loc.ctypes.data_as(fpp), cut.ctypes.data_as(dp), eps)
    comp_args = lambda nb, ns, epsf: (eng._h, fields.ctypes.data_as(dp), 2, F, nb, starts.ctypes.data_as(ip),
                                      pl.ctypes.data_as(ip), fp.ctypes.data_as(C.POINTER(C.c_int64)), n, 1, 2, ns,
                                      fl.ctypes.data_as(dp), fl.ctypes.data_as(dp), epsf, None, None, en.ctypes.data_as(dp))
    with pytest.raises(DvError, match="at least 1"):
        _lib.check(_lib.lib.dv_infer_fields_mc_keep(*keep_args(NB, 0, loc.ctypes.data_as(fpp))))
    with pytest.raises(DvError, match="band 2"):
        _lib.check(_lib.lib.dv_infer_fields_mc_keep(*keep_args(2, 4, loc.ctypes.data_as(fpp))))
    with pytest.raises(DvError, match="must all be given"):
        _lib.check(_lib.lib.dv_infer_fields_mc_keep(*keep_args(NB, 4, None)))
    with pytest.raises(DvError, match="at least 1"):
        _lib.check(_lib.lib.dv_infer_fields_mc_composite(*comp_args(NB, 0, fl.ctypes.data_as(dp))))
    with pytest.raises(DvError, match="band 2"):
        _lib.check(_lib.lib.dv_infer_fields_mc_composite(*comp_args(2, 4, fl.ctypes.data_as(dp))))
    with pytest.raises(DvError, match="must all be given"):
        _lib.check(_lib.lib.dv_infer_fields_mc_composite(*comp_args(NB, 4, None)))
    bad = starts.copy()
    bad[6] = [F - CS + 1, 0]
    with pytest.raises(DvError, match="cutout 6 of field 1"):
        eng.infer_fields_mc_keep(fields, bad, fp, nsamples=4)
    db = DeblendFieldBatch(net, fields)
    with pytest.raises(ValueError, match="epistemic_samples"):
        db.deblend_fields([np.zeros((1, 2)), np.zeros((0, 2))], epistemic_uncertainty_estimation=True, epistemic_samples=0)
    # still usable
    got = eng.infer_fields_mc_keep(fields, starts, fp, seed=3, mc_seed=4, nsamples=4)
    ref = eng.infer_fields_keep(fields, starts, fp, seed=3)
    assert np.array_equal(got["loc"], ref["loc"])
    assert np.array_equal(got["epistemic"], eng.infer_mc(ref["cutouts"].astype(np.float32), 4, seed=4)[1])
    res = db.deblend_fields([np.array([[0.0, 1.0]]), np.zeros((0, 2))], on_device=True, epistemic_uncertainty_estimation=True,
                            epistemic_samples=4)
    assert [len(r) for r in res] == [1, 0] and "epistemic_norm" in res[0].dtype.names
