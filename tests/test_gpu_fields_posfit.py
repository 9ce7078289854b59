"""The sub-pixel position fit and fractional placements inside the on-device many-field call
(dv_infer_fields_fit_composite, DeblendFieldBatch.deblend_fields(on_device=True, optimise_positions=True)).

The fit is compared bit for bit with dv_scene_fit_shifts_fields on the stamps the default path returns, the composited
fields with scipy (oracle.scene_oracle) on those float32 stamps at dist + shifts to 1e-9 absolute - the tolerance of
tests/test_scene.py and tests/test_gpu_posfit.py for the same comparison - and, where 2100 objects make scipy too slow, with
dv_scene_composite, which those tests pin to scipy.  The on-device fields are NOT asserted bit-identical to
dv_scene_composite's: the two kernels share the evaluation function but the compiler is free to contract its multiply-adds
differently in each.  Reference architecture (59 px, 6 bands), fresh weights, max_batch = 64; synthetic blob fields."""
import functools

import numpy as np
import pytest

from oracle import scene_oracle as so

pytestmark = pytest.mark.gpu

ARCH = dict(input_shape=(59, 59, 6), latent_dim=32, filters=[32, 64, 128, 256], kernels=[3, 3, 3, 3])
CS, NB = 59, 6
SEED, MC_SEED, NS = 41, 97, 3
TOL = dict(rtol=0, atol=1e-9)
FIT_KEYS = ("shifts", "objective", "iters", "status")
FIELD_KEYS = ("mean_fields", "stddev_fields", "residual_fields")


def _blob_fields(M, F, seed, nblob=12, amp=(2.0, 9.0), noise=0.05):
    """M fields (M, F, F, 6): Gaussian blobs of random size and flux on Gaussian noise (as tests/test_gpu_fields_batch.py)."""
    rng = np.random.default_rng(seed)
    out = rng.normal(0, noise, size=(M, F, F, NB))
    yy, xx = np.mgrid[:F, :F]
    for m in range(M):
        for _ in range(nblob):
            r, c = rng.uniform(20, F - 20, size=2)
            sig, a = rng.uniform(1.5, 3.5), rng.uniform(*amp)
            g = a * np.exp(-0.5 * ((yy - r) ** 2 + (xx - c) ** 2) / sig ** 2)
            out[m] += g[:, :, None] * rng.uniform(0.5, 1.0, size=NB)
    return out


@functools.lru_cache(maxsize=None)
def _net(dtype):
    from debvader_amd.model import model

    net, _, _, _ = model.create_model_vae(**ARCH, max_batch=64, seed=3, dtype=dtype)
    return net


def _windows(F, counts, seed, reach=None):
    """integer distances to the centre (within +-reach), the cutout starts that go with them, field_ptr"""
    po = int((F - CS) / 2)
    reach = po if reach is None else reach
    rng = np.random.default_rng(seed)
    n = int(np.sum(counts))
    dist = rng.integers(-reach, min(reach, F - CS - po) + 1, size=(n, 2)).astype(np.float64)
    starts = (po + dist).astype(np.int32)
    fp = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return starts, dist, fp


def _oracle_fields(fields, fp, dist, shifts, mean, std, eps=None):
    """scipy: predicted mean / stddev (/ epistemic) and residual fields of the float32 stamps, as float64, at dist + shifts"""
    F = fields.shape[1]
    out = {"mean_fields": np.zeros_like(fields), "stddev_fields": np.zeros_like(fields), "residual_fields": fields.copy()}
    if eps is not None:
        out["epistemic_fields"] = np.zeros_like(fields)
    pos = dist + shifts
    for m in range(len(fields)):
        lo, hi = int(fp[m]), int(fp[m + 1])
        if hi == lo:
            continue
        out["mean_fields"][m] = so.predicted_field(F, NB, mean[lo:hi].astype(np.float64), pos[lo:hi], CS)
        out["stddev_fields"][m] = so.predicted_field(F, NB, std[lo:hi].astype(np.float64), pos[lo:hi], CS)
        out["residual_fields"][m] = so.residual_field(fields[m], mean[lo:hi].astype(np.float64), pos[lo:hi], CS)
        if eps is not None:
            out["epistemic_fields"][m] = so.predicted_field(F, NB, eps[lo:hi].astype(np.float64), pos[lo:hi], CS)
    return out


# case 1: chunks of 64 stamps cross field boundaries (stamps 0 .. 63: fields 0 and 2, 64 .. 81: fields 2 and 3), field 1 is empty
F1, COUNTS1 = 139, [9, 0, 70, 3]


@functools.lru_cache(maxsize=None)
def _case1(dtype):
    eng = _net(dtype)._core.engine
    fields = _blob_fields(4, F1, seed=11)
    starts, dist, fp = _windows(F1, COUNTS1, seed=5)
    out = eng.infer_fields_fit_composite(fields, starts, dist, fp, seed=SEED)
    for v in out.values():
        v.flags.writeable = False
    return fields, starts, dist, fp, out


@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_fit_has_the_bits_of_the_fit_on_the_default_paths_stamps(dtype):
    from debvader_amd.deblend_cutout.optimization import position_optimization_fields

    net = _net(dtype)
    eng = net._core.engine
    fields, starts, dist, fp, out = _case1(dtype)
    keep = eng.infer_fields_keep(fields, starts, fp, seed=SEED)
    sh, det = position_optimization_fields(fields, keep["loc"], dist, fp, bound=3.0, ctx=net._core.ctx, return_details=True)
    np.testing.assert_array_equal(out["shifts"], sh)
    for k in ("objective", "iters", "status"):
        np.testing.assert_array_equal(out[k], det[k], err_msg=k)
    assert np.abs(out["shifts"]).max() > 0.05 and (out["iters"] > 0).any()
    places = (int((F1 - CS) / 2) + dist).astype(np.int64)
    comp = eng.infer_fields_composite(fields, starts, places, fp, seed=SEED)
    np.testing.assert_array_equal(out["mse_center"], comp["mse_center"])


@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_fields_against_scipy_at_the_fitted_positions(dtype):
    eng = _net(dtype)._core.engine
    fields, starts, dist, fp, out = _case1(dtype)
    mck = eng.infer_fields_mc_keep(fields, starts, fp, seed=SEED, mc_seed=MC_SEED, nsamples=NS)
    mc = eng.infer_fields_fit_composite(fields, starts, dist, fp, seed=SEED, mc_seed=MC_SEED, nsamples=NS)
    for k in FIT_KEYS + FIELD_KEYS + ("mse_center",):        # the Monte-Carlo stage changes nothing else
        np.testing.assert_array_equal(mc[k], out[k], err_msg=k)
    frac = (out["shifts"] != np.floor(out["shifts"])).any(axis=1)
    assert frac.sum() > 10                                      # the spline path is what is compared
    exp = _oracle_fields(fields, fp, dist, out["shifts"], mck["loc"], mck["scale"], mck["epistemic"])
    for k in FIELD_KEYS + ("epistemic_fields",):
        np.testing.assert_allclose(mc[k], exp[k], err_msg=k, **TOL)
    assert not mc["mean_fields"][1].any() and np.array_equal(mc["residual_fields"][1], fields[1])
    eps64 = mck["epistemic"].astype(np.float64)
    np.testing.assert_allclose(mc["eps_norm"], eps64[..., 2].sum(axis=(1, 2)) / mck["loc"].astype(np.float64)[..., 2].sum(axis=(1, 2)),
                               rtol=1e-10, atol=0)


def test_mirror_terms_and_stamps_on_the_fields_edge():
    # po = 8 < T_MARGIN + 2: the coefficients reflected at the field's edge samples contribute
    eng = _net("float32")._core.engine
    F = 75
    fields = _blob_fields(2, F, seed=21, nblob=5)
    starts, dist, fp = _windows(F, [5, 2], seed=6, reach=8)
    dist[0], dist[1], dist[2] = (-8, 8), (8, -8), (-8, -8)      # stamps touch the field's edges
    starts = (8 + dist).astype(np.int32)
    rng = np.random.default_rng(8)
    start = np.array([(0, 0), (3, -3), (0.5, 0), (-2.25, 1.75), (-3, 2.5)] + list(rng.uniform(-3, 3, size=(2, 2))))
    out = eng.infer_fields_fit_composite(fields, starts, dist, fp, seed=SEED, shifts=start, max_iter=0)
    np.testing.assert_array_equal(out["shifts"], start)
    assert (out["status"] == 2).all() and not out["iters"].any()
    keep = eng.infer_fields_keep(fields, starts, fp, seed=SEED)
    exp = _oracle_fields(fields, fp, dist, start, keep["loc"], keep["scale"])
    for k in FIELD_KEYS:
        np.testing.assert_allclose(out[k], exp[k], err_msg=k, **TOL)
    # the M = 1 wrapper on the first field: the many-field call's bits under singular names, and the same fields
    one = eng.infer_cutouts_fit_composite(fields[0], starts[:5], dist[:5], seed=SEED, shifts=start[:5], max_iter=0)
    same = eng.infer_fields_fit_composite(fields[:1], starts[:5], dist[:5], [0, 5], seed=SEED, shifts=start[:5], max_iter=0)
    for k in FIELD_KEYS:
        np.testing.assert_array_equal(one[k[:-1]], same[k][0], err_msg=k)
        np.testing.assert_allclose(one[k[:-1]], exp[k][0], err_msg=k, **TOL)


@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_zero_shifts_give_the_integer_calls_fields(dtype):
    eng = _net(dtype)._core.engine
    fields, starts, dist, fp, _ = _case1(dtype)
    places = (int((F1 - CS) / 2) + dist).astype(np.int64)
    comp = eng.infer_fields_composite(fields, starts, places, fp, seed=SEED)
    out = eng.infer_fields_fit_composite(fields, starts, dist, fp, seed=SEED, max_iter=0)
    for k in FIELD_KEYS + ("mse_center",):
        np.testing.assert_array_equal(out[k], comp[k], err_msg=k)
    assert not out["shifts"].any()


def test_more_than_2048_fractional_objects_on_one_tile():
    net = _net("float32")
    eng, ctx = net._core.engine, net._core.ctx
    F, n = 75, 2100
    fields = _blob_fields(1, F, seed=31, nblob=4)
    dist = np.tile(np.array([[2.0, -3.0]]), (n, 1))
    starts = (8 + dist).astype(np.int32)
    fp = np.array([0, n], np.int64)
    start = np.random.default_rng(9).uniform(-3, 3, size=(n, 2))
    out = eng.infer_fields_fit_composite(fields, starts, dist, fp, seed=SEED, shifts=start, max_iter=0)
    keep = eng.infer_fields_keep(fields, starts, fp, seed=SEED)
    pos = dist + start
    zeros = np.zeros(fields.shape[1:])
    loc = keep["loc"].astype(np.float64)
    np.testing.assert_allclose(out["mean_fields"][0], ctx.scene_composite(zeros, loc, pos), **TOL)
    np.testing.assert_allclose(out["residual_fields"][0], ctx.scene_composite(fields[0], loc, pos, -1.0), **TOL)
    del loc
    np.testing.assert_allclose(out["stddev_fields"][0], ctx.scene_composite(zeros, keep["scale"].astype(np.float64), pos), **TOL)


def test_same_bits_on_every_run_and_for_any_grouping(monkeypatch):
    eng = _net("float32")._core.engine
    fields, starts, dist, fp, out = _case1("float32")
    again = eng.infer_fields_fit_composite(fields, starts, dist, fp, seed=SEED)
    for k in out:
        np.testing.assert_array_equal(again[k], out[k], err_msg=k)
    # a resident field takes four 0.93-MB buffers and its 0.15-MB r-band plane, 3.9 MB: 12 MB hold three, so chunk 0 runs
    # with fields 0-2 resident, chunk 1 with fields 2-3, and field 2's sums travel from one group to the next
    monkeypatch.setenv("DV_FIELDS_GROUP_MB", "12")
    grouped = eng.infer_fields_fit_composite(fields, starts, dist, fp, seed=SEED)
    monkeypatch.delenv("DV_FIELDS_GROUP_MB")
    for k in out:
        np.testing.assert_array_equal(grouped[k], out[k], err_msg=k)


def _device_against_host(net, fields, dists):
    """deblend_fields(on_device=True, optimise_positions=True) against a second object's default pass with
    optimise_positions=True from the same seed counter: shifts bit for bit, fields to 1e-9"""
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch

    M = len(fields)
    counter = net._core.seed_counter
    dev = DeblendFieldBatch(net, fields)
    res = dev.deblend_fields(dists, on_device=True, optimise_positions=True)
    after = net._core.seed_counter
    net._core.seed_counter = counter                            # the second object draws the same seed
    host = DeblendFieldBatch(net, fields)
    ref = host.deblend_fields(dists, optimise_positions=True)
    assert net._core.seed_counter == after == counter + 1       # one seed per pass, with or without the fit
    assert [r.dtype.names for r in res] == [tuple(n for n, _ in DeblendFieldBatch.ON_DEVICE_COLUMNS)] * M
    for m in range(M):
        assert len(res[m]) == len(dists[m]) == len(dev.position_fit[m]["status"])
        for a, b in zip(res[m]["shifts"], ref[m]["shifts"]):
            assert a.dtype == np.float64 and np.array_equal(a, b)
        np.testing.assert_array_equal(res[m]["passed_cuts"], ref[m]["passed_cuts"])
    assert max(np.abs(s).max() for r in res for s in r["shifts"]) > 0.05
    pd, ph = dev.get_predicted_fields(), host.get_predicted_fields()
    for k in ("predicted_mean_fields", "predicted_stddev_fields"):
        np.testing.assert_allclose(pd[k], ph[k], err_msg=k, **TOL)
    np.testing.assert_allclose(dev.get_residual_fields(), host.get_residual_fields(), **TOL)
    return dev, res


def test_deblend_field_batch_fits_on_the_device_what_the_default_path_fits_on_the_host():
    net = _net("float32")
    fields = _blob_fields(3, 139, seed=51)
    rng = np.random.default_rng(12)
    dists = [rng.integers(-30, 31, size=(n, 2)).astype(np.float64) for n in (6, 0, 11)]
    _device_against_host(net, fields, dists)
    # M = 1 (its six stamps are a list of their own: a call of its own size on both paths)
    one, r1 = _device_against_host(net, fields[:1], dists[:1])
    # a refused call leaves the engine usable: the same pass again gives the same bits
    counter = net._core.seed_counter
    with pytest.raises(ValueError, match="integer"):
        one.deblend_fields([dists[0] + 0.5], on_device=True, optimise_positions=True)
    net._core.seed_counter = counter - 1
    before = one.get_predicted_fields()["predicted_mean_fields"]
    r2 = one.deblend_fields(dists[:1], on_device=True, optimise_positions=True)
    for a, b in zip(r2[0]["shifts"], r1[0]["shifts"]):
        assert np.array_equal(a, b)
    np.testing.assert_array_equal(one.get_predicted_fields()["predicted_mean_fields"], before)
