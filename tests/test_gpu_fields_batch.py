"""Many fields in one engine call (dv_infer_fields, _keep, _composite, dv_scene_fit_shifts_fields, DeblendFieldBatch) against
the single-field and stamp-level entry points they batch.  Every comparison is bit for bit: the expected values come from
entry points the header promises to be bit-identical to each other (dv_scene_extract -> dv_infer_f64, dv_scene_composite in
object order, dv_scene_fit_shifts per field).  Inputs are synthetic six-band fields (Gaussian blobs on noise) built here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ARCH = dict(input_shape=(59, 59, 6), latent_dim=32, filters=[32, 64, 128, 256], kernels=[3, 3, 3, 3])
CS, NB = 59, 6
WANT = ("loc", "scale", "mu", "zstd", "z")


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


def _case(F, counts, seed, hang=True):
    """starts / places / field_ptr for fields with `counts` stamps each: windows anywhere inside the field, placements
    anywhere that keeps at least a corner of the stamp near the field - some hang over its edges"""
    rng = np.random.default_rng(seed)
    n = int(np.sum(counts))
    starts = rng.integers(0, F - CS + 1, size=(n, 2)).astype(np.int32)
    places = starts.copy()
    if hang:
        k = rng.random(n) < 0.3
        places[k] = rng.integers(-CS + 3, F - 3, size=(int(k.sum()), 2))
    fp = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return starts, places, fp


def _expected_stamps(net, fields, starts, fp, seed):
    """ctx.scene_extract per field, concatenated in field order, then engine.infer on the cutouts"""
    ctx, eng = net._core.ctx, net._core.engine
    cut = [ctx.scene_extract(fields[m], starts[fp[m]:fp[m + 1]], CS) for m in range(len(fields)) if fp[m + 1] > fp[m]]
    cut = np.concatenate(cut) if cut else np.zeros((0, CS, CS, NB))
    return cut, eng.infer(cut, seed=seed, want=WANT)


def _expected_fields(net, fields, exp, places, fp):
    """ctx.scene_composite of the expected float32 stamps (as float64) per field, in object order"""
    ctx = net._core.ctx
    F = fields.shape[1]
    po = int((F - CS) / 2)
    mean, std, res = np.zeros_like(fields), np.zeros_like(fields), fields.copy()
    zeros = np.zeros(fields.shape[1:])
    for m in range(len(fields)):
        lo, hi = int(fp[m]), int(fp[m + 1])
        if hi == lo:
            continue
        pos = (places[lo:hi] - po).astype(np.float64)
        loc, scale = exp["loc"][lo:hi].astype(np.float64), exp["scale"][lo:hi].astype(np.float64)
        mean[m] = ctx.scene_composite(zeros, loc, pos)
        std[m] = ctx.scene_composite(zeros, scale, pos)
        res[m] = ctx.scene_composite(fields[m], loc, pos, -1.0)
    return mean, std, res


def _host_mse(cut, loc):
    """DeblendField's host formula (field_deblender.py: metrics.mse of the centre 10 x 10 pixels)"""
    c0, c1 = int(CS / 2) - 5, int(CS / 2) + 5
    diff = cut[:, c0:c1, c0:c1] - loc[:, c0:c1, c0:c1]
    return np.mean(np.square(diff).reshape(len(diff), -1), axis=1)


COUNTS = [30, 0, 150, 7, 40]      # one empty field, one with more stamps than max_batch = 64: chunks cross field boundaries


@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_network_outputs_and_composited_fields_equal_the_stamp_level_path(dtype, monkeypatch):
    net = _net(dtype)
    eng = net._core.engine
    F = 131
    fields = _blob_fields(5, F, seed=11)
    starts, places, fp = _case(F, COUNTS, seed=5)
    # fields 0 and 4: objects at the same coordinates (the first 30 of field 4 repeat field 0's)
    starts[fp[4]:fp[4] + 30], places[fp[4]:fp[4] + 30] = starts[:30], places[:30]
    assert (places < 0).any() and (places > F - CS).any()          # stamps hang over the edges
    seed = 77
    cut, exp = _expected_stamps(net, fields, starts, fp, seed)

    # 1. network outputs
    got = eng.infer_fields(fields, starts, fp, seed=seed, want=WANT)
    for k in WANT:
        assert got[k].shape == exp[k].shape
        assert np.array_equal(got[k], exp[k]), k
    keep = eng.infer_fields_keep(fields, starts, fp, seed=seed, want=WANT)
    for k in WANT:
        assert np.array_equal(keep[k], exp[k]), k
    assert keep["cutouts"].dtype == np.float64 and np.array_equal(keep["cutouts"], cut)

    # 2. composited fields and the centre MSE
    mean, std, res = _expected_fields(net, fields, exp, places, fp)
    out = eng.infer_fields_composite(fields, starts, places, fp, seed=seed)
    assert np.array_equal(out["mean_fields"], mean)
    assert np.array_equal(out["stddev_fields"], std)
    assert np.array_equal(out["residual_fields"], res)
    assert np.array_equal(out["mse_center"], _host_mse(cut, exp["loc"]))
    assert not out["mean_fields"][1].any() and np.array_equal(out["residual_fields"][1], fields[1])
    assert np.abs(mean[0]).max() > 0 and not np.array_equal(mean[0], mean[4])
    # without the optional outputs
    part = eng.infer_fields_composite(fields, starts, places, fp, seed=seed, residual=False, mse_center=False)
    assert sorted(part) == ["mean_fields", "stddev_fields"] and np.array_equal(part["mean_fields"], mean)

    # the same with the fields uploaded in groups of three (10 MB of four 0.8-MB buffers per field): chunks 0-1 run with
    # fields 0-2 resident, chunks 2-3 with fields 2-4, and field 2's sums travel from one group to the next
    monkeypatch.setenv("DV_FIELDS_GROUP_MB", "10")
    grouped = eng.infer_fields_composite(fields, starts, places, fp, seed=seed)
    for k in out:
        assert np.array_equal(grouped[k], out[k]), k
    monkeypatch.setenv("DV_FIELDS_GROUP_MB", "3")         # three 0.8-MB fields at a time
    g2 = eng.infer_fields_keep(fields, starts, fp, seed=seed, want=WANT)
    for k in g2:
        assert np.array_equal(g2[k], keep[k]), k
    # a group that cannot hold one field (its four buffers need 3.3 MB), or the three fields of chunk 0: refused
    monkeypatch.setenv("DV_FIELDS_GROUP_MB", "1")
    from debvader_amd._lib import DvError
    with pytest.raises(DvError, match="needs"):
        eng.infer_fields_composite(fields, starts, places, fp, seed=seed)
    monkeypatch.setenv("DV_FIELDS_GROUP_MB", "7")
    with pytest.raises(DvError, match="lower max_batch"):
        eng.infer_fields_composite(fields, starts, places, fp, seed=seed)
    monkeypatch.delenv("DV_FIELDS_GROUP_MB")

    # normalise=True runs through the same forward pass
    eng.set_normalise(True)
    try:
        a = eng.infer_fields_composite(fields[:1], starts[:30], places[:30], fp[:2], seed=seed)
        b = eng.infer_cutouts_composite(fields[0], starts[:30], places[:30], seed=seed)
    finally:
        eng.set_normalise(False)
    assert np.array_equal(a["mean_fields"][0], b["mean_field"]) and not np.array_equal(b["mean_field"], mean[0])

    # 3. M = 1 is infer_cutouts_composite on that field
    s1, p1, fp1 = _case(F, [150], seed=9)
    one = eng.infer_fields_composite(fields[2:3], s1, p1, fp1, seed=seed)
    ref = eng.infer_cutouts_composite(fields[2], s1, p1, seed=seed)
    assert np.array_equal(one["mean_fields"][0], ref["mean_field"])
    assert np.array_equal(one["stddev_fields"][0], ref["stddev_field"])
    assert np.array_equal(one["residual_fields"][0], ref["residual_field"])
    assert np.array_equal(one["mse_center"], ref["mse_center"])

    # 4. a field's result does not depend on the other fields' pixels, and a second run gives the same bits
    again = eng.infer_fields_composite(fields, starts, places, fp, seed=seed)
    for k in out:
        assert np.array_equal(again[k], out[k]), k
    other = _blob_fields(5, F, seed=12)
    other[2] = fields[2]
    o2 = eng.infer_fields_composite(other, starts, places, fp, seed=seed)
    for k in ("mean_fields", "stddev_fields", "residual_fields"):
        assert np.array_equal(o2[k][2], out[k][2]), k
        assert not np.array_equal(o2[k][0], out[k][0]), k
    assert np.array_equal(o2["mse_center"][fp[2]:fp[3]], out["mse_center"][fp[2]:fp[3]])


@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_centre_mse_equals_the_host_formula_bit_for_bit(dtype):
    """mse_center of infer_fields_composite against DeblendField's host formula (numpy: mean of the squared differences
    over the centre 10 x 10 pixels and all bands) on the expected stamps, bit for bit: the kernel adds the 600 squares in
    numpy's pairwise order.  The single-field call runs the same kernel, so it gives these bits too."""
    net = _net(dtype)
    eng = net._core.engine
    F = 131
    fields = _blob_fields(5, F, seed=11)
    starts, places, fp = _case(F, COUNTS, seed=5)
    cut, exp = _expected_stamps(net, fields, starts, fp, 77)
    out = eng.infer_fields_composite(fields, starts, places, fp, seed=77)
    want = _host_mse(cut, exp["loc"])
    rel = np.abs(out["mse_center"] - want) / want
    print(f"mse_center vs host formula [{dtype}]: {int((out['mse_center'] != want).sum())} of {len(want)} differ, "
          f"max relative difference {rel.max():.3e}")
    assert np.array_equal(out["mse_center"], want)
    one = eng.infer_cutouts_composite(fields[0], starts[:30], places[:30], seed=77)      # stamps 0 .. 29: the same noise rows
    assert np.array_equal(one["mse_center"], want[:30])


@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_a_pile_of_more_than_2048_objects_on_one_tile(dtype):
    """max_batch = 2560 and 5200 stamps: chunks of 2560, so the 2100 objects piled on one spot of field 0 take more than one
    2048-object scan round of one chunk; field 1's 3000 scattered objects cross the chunk boundary, field 2 has 100."""
    net = _net(dtype, max_batch=2560)
    eng = net._core.engine
    F = 131
    fields = _blob_fields(3, F, seed=21)
    starts, places, fp = _case(F, [2100, 3000, 100], seed=6)
    starts[:2100], places[:2100] = [40, 17], [45, 30]
    seed = 5
    cut, exp = _expected_stamps(net, fields, starts, fp, seed)
    mean, std, res = _expected_fields(net, fields, exp, places, fp)
    out = eng.infer_fields_composite(fields, starts, places, fp, seed=seed)
    assert np.array_equal(out["mean_fields"], mean)
    assert np.array_equal(out["stddev_fields"], std)
    assert np.array_equal(out["residual_fields"], res)
    assert np.array_equal(out["mse_center"], _host_mse(cut, exp["loc"]))


def _gauss(cs, sig, amp, c=(0.0, 0.0)):
    y, x = np.mgrid[:cs, :cs] - (cs - 1) / 2.0
    return amp * np.exp(-0.5 * (((x - c[1]) / sig) ** 2 + ((y - c[0]) / sig) ** 2))


def test_position_fit_on_many_fields_equals_the_fit_field_by_field(monkeypatch):
    from debvader_amd import engine as E

    ctx = E.default_context()
    rng = np.random.default_rng(8)
    M, F, cs = 9, 131, 31
    counts = [4, 0, 7, 1, 3, 5, 0, 2, 6]
    fp = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    n = int(fp[-1])
    fields = rng.normal(0, 0.05, size=(M, F, F))
    dist = np.round(rng.uniform(-40, 40, size=(n, 2)))
    dist[::3] += rng.uniform(-0.5, 0.5, size=dist[::3].shape)          # fractional distances too
    stamps = np.array([_gauss(cs, rng.uniform(2, 4), rng.uniform(2, 6)) for _ in range(n)])
    po = int((F - cs) / 2)
    for m in range(M):                    # every field holds its galaxies, displaced by a sub-pixel shift to be found
        for i in range(int(fp[m]), int(fp[m + 1])):
            r, c = po + int(np.floor(dist[i, 0])), po + int(np.floor(dist[i, 1]))
            fields[m, r:r + cs, c:c + cs] += _gauss(cs, 3.0, 4.0, c=rng.uniform(-1.5, 1.5, size=2))
    start = rng.uniform(-0.5, 0.5, size=(n, 2))
    keys = ("shifts", "objective", "iters", "status")
    exp = {k: [] for k in keys}
    for m in range(M):
        lo, hi = int(fp[m]), int(fp[m + 1])
        r = ctx.scene_fit_shifts(fields[m], stamps[lo:hi], dist[lo:hi], shifts=start[lo:hi])
        for k in keys:
            exp[k].append(r[k])
    got = ctx.scene_fit_shifts_fields(fields, stamps, dist, fp, shifts=start)
    for k in keys:
        assert np.array_equal(got[k], np.concatenate(exp[k])), k
    assert np.abs(got["shifts"]).max() > 0.1
    # seven 137-KB r-band fields per MB: two groups
    monkeypatch.setenv("DV_FIELDS_GROUP_MB", "1")
    grouped = ctx.scene_fit_shifts_fields(fields, stamps, dist, fp, shifts=start)
    for k in keys:
        assert np.array_equal(grouped[k], got[k]), k
    # the objective alone (max_iter = 0), and the module-level form on six-band fields
    from debvader_amd.deblend_cutout.optimization import position_optimization_fields

    six = np.zeros((M, F, F, NB))
    six[..., 2] = fields
    s6 = np.zeros((n, cs, cs, NB))
    s6[..., 2] = stamps
    monkeypatch.delenv("DV_FIELDS_GROUP_MB")
    sh, det = position_optimization_fields(six, s6, dist, fp, ctx=ctx, return_details=True)
    zero = ctx.scene_fit_shifts_fields(fields, stamps, dist, fp)
    assert np.array_equal(sh, zero["shifts"]) and np.array_equal(det["objective"], zero["objective"])


@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_class_detects_deblends_and_both_modes_give_the_same_fields(dtype):
    from debvader_amd.deblend.field_deblender import DeblendField, DeblendFieldBatch
    from debvader_amd.detect.detection import detect_objects
    from debvader_amd.extract.extraction import cutout_windows

    net = _net(dtype)
    M, F = 4, 160
    fields = _blob_fields(M, F, seed=31, nblob=9)
    fields[3] = np.random.default_rng(1).normal(0, 0.05, size=(F, F, NB))        # nothing to detect here
    a = DeblendFieldBatch(net, fields)
    net._core.seed_counter = 500
    res = a.deblend_fields(None)
    assert net._core.seed_counter == 501                     # one pass, one seed
    ra, pa = a.get_residual_fields(), a.get_predicted_fields()
    b = DeblendFieldBatch(net, fields)
    net._core.seed_counter = 500
    rb = b.deblend_fields(None, on_device=True)
    rfb, pb = b.get_residual_fields(), b.get_predicted_fields()
    assert len(res) == M and len(rb) == M and sum(len(r) for r in res) >= 12
    for m in range(M):
        d = np.asarray(detect_objects(fields[m:m + 1], ctx=net._core.ctx), dtype=np.float64).reshape(-1, 2)
        ok = cutout_windows(F, d, CS)[1] if len(d) else np.zeros(0, bool)
        for r in (res[m], rb[m]):
            assert np.array_equal(r["list_idx"], np.nonzero(ok)[0])
            assert np.array_equal(r["galaxy_distances_to_center_x"], d[ok, 0])
            assert np.array_equal(r["galaxy_distances_to_center_y"], d[ok, 1])
        assert list(res[m]["passed_cuts"]) == list(rb[m]["passed_cuts"])
    assert np.array_equal(rfb, ra)
    assert np.array_equal(pb["predicted_mean_fields"], pa["predicted_mean_fields"])
    assert np.array_equal(pb["predicted_stddev_fields"], pa["predicted_stddev_fields"])
    assert np.abs(pa["predicted_mean_fields"]).max() > 0 and ra.shape == fields.shape
    # a single field through the batch class is DeblendField on that field
    m = int(np.argmax([len(r) for r in res]))
    d = np.stack([res[m]["galaxy_distances_to_center_x"], res[m]["galaxy_distances_to_center_y"]], axis=1)
    one = DeblendFieldBatch(net, fields[m:m + 1])
    net._core.seed_counter = 40
    one.deblend_fields([d], on_device=True)
    single = DeblendField(net, fields[m:m + 1])
    net._core.seed_counter = 40
    rs = single.deblend_field(d, on_device=True)
    assert np.array_equal(one.get_residual_fields(), single.get_residual_field())
    assert np.array_equal(one.res_deblend[0]["mse_center"], rs["mse_center"])
    # the position fit of all rows in one call writes the shifts DeblendField.optimise_positions writes field by field
    a.optimise_positions()
    for m in range(M):
        if len(res[m]) == 0:
            continue
        s = DeblendField(net, fields[m:m + 1])
        rec = s.optimise_positions(res[m].copy())
        assert all(np.array_equal(x, y) for x, y in zip(a.res_deblend[m]["shifts"], rec["shifts"]))
    assert any(np.abs(x).max() > 0 for r in a.res_deblend for x in r["shifts"])


def test_refusals_leave_the_engine_usable():
    from debvader_amd._lib import DvError
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch

    net = _net("float32")
    eng = net._core.engine
    F = 131
    fields = _blob_fields(2, F, seed=41)
    starts, places, fp = _case(F, [5, 3], seed=2)
    with pytest.raises(ValueError, match="field_ptr"):
        eng.infer_fields(fields, starts, [0, 5, 7])
    with pytest.raises(ValueError, match="field_ptr"):
        eng.infer_fields_composite(fields, starts, places, [0, 9, 8])
    with pytest.raises(ValueError, match="field_ptr"):
        eng.infer_fields_keep(fields, starts, [0, 8])
    bad = starts.copy()
    bad[6] = [F - CS + 1, 0]
    with pytest.raises(DvError, match="cutout 6 of field 1"):
        eng.infer_fields(fields, bad, fp)
    with pytest.raises(DvError, match="leaves the 131-pixel field"):
        eng.infer_fields_composite(fields, bad, places, fp)
    with pytest.raises(DvError, match="network takes"):
        eng.infer_fields(fields[:, :, :, :3], starts, fp)
    db = DeblendFieldBatch(net, fields)
    with pytest.raises(ValueError, match="integer positions"):
        db.deblend_fields([np.array([[0.5, 1.0]]), np.zeros((0, 2))], on_device=True)
    ctx = net._core.ctx
    with pytest.raises(ValueError, match="field_ptr"):
        ctx.scene_fit_shifts_fields(fields[..., 2], np.zeros((2, 31, 31)), np.zeros((2, 2)), [0, 1, 3])
    # still usable
    got = eng.infer_fields(fields, starts, fp, seed=3)
    cut, exp = _expected_stamps(net, fields, starts, fp, 3)
    assert np.array_equal(got["loc"], exp["loc"])
    res = db.deblend_fields([np.array([[0.0, 1.0]]), np.zeros((0, 2))], on_device=True)
    assert [len(r) for r in res] == [1, 0]
