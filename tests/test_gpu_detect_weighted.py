"""The GPU source detector with a per-pixel noise map and a mask (Context.scene_detect(weights=..., mask=...),
dv_scene_detect_weighted, FieldSet.set_detect_weights) against its numpy restatement
(tests/detect_weighted_oracle.py), against the unweighted detector where the section promises its bits, and through the
resident set and the iterative loop.  Tolerances against the oracle are those of tests/test_gpu_detect.py."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from tests import detect_weighted_oracle as wo
from tests.test_gpu_detect import _blends, _gauss

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CAT = ("field", "parent", "npix", "peak", "flux", "x", "y")
MAPS = ("back", "rms", "D", "labels")


def _ctx():
    from debvader_amd import engine as E
    return E.default_context()


def _golden():
    return np.load(os.path.join(HERE, "golden", "detect.npz"))


def _compare(got, i, exp):
    """field i of a weighted scene_detect result with maps against the oracle's detect() of the same field"""
    for k in ("back", "rms", "D"):
        g, e = got[k][i], exp[k]
        np.testing.assert_array_equal(np.isneginf(g), np.isneginf(e), err_msg=k)
        np.testing.assert_array_equal(np.isnan(g), np.isnan(e), err_msg=k)
        fin = np.isfinite(e)
        assert np.isfinite(g[fin]).all() and not np.isposinf(g).any(), k
        scale = np.abs(e[fin]).max()
        err = np.abs(g[fin] - e[fin]).max()
        print(f"{k}: max error {err:.3e}, bound {1e-12 * scale:.3e}")
        assert err <= 1e-12 * scale, k
    np.testing.assert_allclose(got["globalrms"][i], exp["globalrms"], rtol=1e-12, atol=0)
    np.testing.assert_array_equal(got["labels"][i], exp["labels"])
    assert got["bad_meshes"][i] == exp["bad_meshes"]
    lo, hi = got["offsets"][i], got["offsets"][i + 1]
    assert hi - lo == len(exp["x"]), (hi - lo, len(exp["x"]))
    assert (got["field"][lo:hi] == i).all()
    np.testing.assert_array_equal(got["npix"][lo:hi], exp["npix"])
    np.testing.assert_array_equal(got["parent"][lo:hi], exp["parent"])
    for k in ("peak", "flux"):
        scale = max(np.abs(exp[k]).max(), 1e-300) if len(exp[k]) else 1.0
        np.testing.assert_allclose(got[k][lo:hi], exp[k], rtol=0, atol=1e-12 * scale, err_msg=k)
    for k in ("x", "y"):
        np.testing.assert_allclose(got[k][lo:hi], exp[k], rtol=0, atol=1e-9, err_msg=k)


def _same_bits(a, b, keys=None):
    for k in keys or a:
        assert k in b, k
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        assert a[k].dtype == b[k].dtype, k


def _check(field, weights, **kw):
    got = _ctx().scene_detect(field[None], weights=weights[None], return_maps=True, **kw)
    exp = wo.detect(field, weights, **{"noise": "absolute", **kw})
    _compare(got, 0, exp)
    return got, exp


SETTINGS = [dict(filter_type="conv", noise="absolute", thresh=1.5), dict(filter_type="matched", noise="absolute", thresh=5.0),
            dict(filter_type="conv", noise="relative", thresh=1.5)]


@pytest.mark.parametrize("kw", SETTINGS, ids=["conv-absolute", "matched-absolute", "mask-relative"])
def test_scene_with_defects_stage_by_stage(kw):
    data, weights, mask, planted = wo.scene()
    w = np.where(mask, 0.0, 1.0) if kw["noise"] == "relative" else weights
    got, exp = _check(data, w, back_size=32, **kw)
    assert len(exp["x"]) == 6 and exp["bad_meshes"] == 1
    d = np.hypot(planted[:, 0][:, None] - got["y"][None], planted[:, 1][:, None] - got["x"][None])
    assert (d.min(axis=1) <= 1.0).all()
    if kw["noise"] == "relative":                      # the same call through mask= alone
        m = _ctx().scene_detect(data[None], mask=mask[None], return_maps=True, back_size=32)
        _same_bits(got, m)


def test_field_smaller_than_one_mesh_with_a_stripe_and_a_non_square_kernel():
    rng = np.random.default_rng(6)
    small = 3.0 + rng.normal(0, 2.0, (40, 50)) + _gauss((40, 50), 20, 25, 2.0, 60.0) + _gauss((40, 50), 8, 40, 1.5, 50.0)
    w = np.full((40, 50), 0.25)
    w[:, 30] = 0.0                                      # a masked stripe, three columns from the first source
    w[12, :8] = np.nan
    small[12, :8] = np.nan
    kern = np.outer([1.0, 2.0, 1.0], [1.0, 3.0, 4.0, 3.0, 1.0])
    for kw in SETTINGS[:2]:
        got, exp = _check(small, w, filter_kernel=kern, **kw)
        assert len(exp["x"]) >= 2 and exp["bad_meshes"] == 0
    assert np.isneginf(got["D"][0][:, 30]).all()


@functools.lru_cache(maxsize=None)
def _unweighted(name):
    f = _blends(200, 259, 4) if name == "blends" else _golden()["field2_r"].astype(np.float64)
    return f, _ctx().scene_detect(f[None], return_maps=True)


@pytest.mark.parametrize("name", ["blends", "dc2"])
def test_unit_weights_have_the_bits_of_scene_detect(name):
    f, ref = _unweighted(name)
    assert len(ref["x"]) > 5
    ctx = _ctx()
    ones = np.ones_like(f)[None]
    rel = ctx.scene_detect(f[None], weights=ones, noise="relative", return_maps=True)
    _same_bits(ref, rel)
    assert rel["bad_meshes"].tolist() == [0]
    ab = ctx.scene_detect(f[None], weights=ones, thresh=1.5 * ref["globalrms"][0], return_maps=True)    # noise: absolute
    _same_bits(ref, ab)
    m = ctx.scene_detect(f[None], mask=np.zeros(ones.shape, bool), return_maps=True)
    _same_bits(ref, m)


def test_masked_values_reach_no_sum():
    data, weights, mask, _ = wo.scene()
    ctx = _ctx()
    for kw in SETTINGS[:2]:
        ref = ctx.scene_detect(data[None], weights=weights[None], return_maps=True, back_size=32, **kw)
        assert len(ref["x"]) == 6
        for val in (np.nan, np.inf, -np.inf, 1e300):
            d = data.copy()
            d[mask] = val
            got = ctx.scene_detect(d[None], weights=weights[None], return_maps=True, back_size=32, **kw)
            _same_bits(ref, got)


def test_weighted_component_above_the_lds_budget_takes_the_global_path():
    rng = np.random.default_rng(7)
    sigma = np.where(np.arange(256) < 128, 1.0, 2.0)[None, :] * np.ones((256, 1))
    f = rng.normal(0, 1, (256, 256)) * sigma + _gauss((256, 256), 120, 110, 15.0, 100.0) + \
        _gauss((256, 256), 126, 150, 10.0, 80.0) + _gauss((256, 256), 30, 200, 2.0, 20.0)
    w = 1.0 / sigma ** 2
    w[200:, 17] = 0.0
    f[200:, 17] = np.inf
    got, exp = _check(f, w)
    assert exp["npix"].max() > 2048 and len(exp["x"]) >= 3
    big = exp["parent"][np.argmax(exp["npix"])]
    assert (exp["labels"] == big).sum() > 2048 and (exp["parent"] == big).sum() >= 2


def _three():
    data, weights, mask, _ = wo.scene()
    fields = np.stack([data, np.nan_to_num(_blends(96, 120, 8), nan=0.0), np.nan_to_num(data[::-1], nan=1.0)])
    w = np.stack([weights, np.ones_like(weights), weights[::-1]])
    return fields, w


def _need(msg):
    m = re.search(r"needs up to (\d+) bytes", msg)
    assert m, msg
    return int(m.group(1))


def test_bit_reproducible_independent_of_the_batch_and_of_the_workspace():
    from debvader_amd._lib import DvError

    fields, w = _three()
    ctx = _ctx()
    kw = dict(return_maps=True, back_size=32)
    a = ctx.scene_detect(fields, weights=w, **kw)
    assert (np.diff(a["offsets"]) > 0).all()
    b = ctx.scene_detect(fields, weights=w, **kw)
    _same_bits(a, b)
    for i in range(3):
        one = ctx.scene_detect(fields[i:i + 1], weights=w[i:i + 1], **kw)
        lo, hi = a["offsets"][i], a["offsets"][i + 1]
        for k in CAT[1:]:
            np.testing.assert_array_equal(one[k], a[k][lo:hi], err_msg=k)
        for k in MAPS:
            np.testing.assert_array_equal(one[k][0], a[k][i], err_msg=k)
        assert one["globalrms"][0] == a["globalrms"][i] and one["bad_meshes"][0] == a["bad_meshes"][i]
    # what one field needs, as the refusal names it; the weight plane and the bad-mesh count are counted
    with pytest.raises(DvError, match="workspace") as weighted:
        ctx.scene_detect(fields, weights=w, workspace_bytes=1, **kw)
    with pytest.raises(DvError, match="workspace") as plain:
        ctx.scene_detect(np.nan_to_num(fields), workspace_bytes=1, **kw)
    need = _need(str(weighted.value))
    assert need - _need(str(plain.value)) == 96 * 120 * 8 + 4
    c = ctx.scene_detect(fields, weights=w, workspace_bytes=need, **kw)          # one field per launch
    _same_bits(a, c)
    with pytest.raises(DvError, match="workspace") as below:
        ctx.scene_detect(fields, weights=w, workspace_bytes=need - 1, **kw)
    assert _need(str(below.value)) == need
    _same_bits(a, ctx.scene_detect(fields, weights=w, **kw))


def test_refusals_leave_the_engine_usable():
    from debvader_amd import _lib
    from debvader_amd._lib import DvError

    data, weights, _, _ = wo.scene()
    ctx = _ctx()
    ref = ctx.scene_detect(data[None], weights=weights[None], back_size=32)
    f = np.ascontiguousarray(np.nan_to_num(data)[None])
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    n, off, g = C.c_int64(), np.zeros(2, np.int64), np.zeros(1)

    def call(thresh, wstruct):
        p = _lib.DvDetectParams(thresh, 1e-5, 4, 64, 32, 3, None, 0, 0, 0)
        return _lib.lib.dv_scene_detect_weighted(ctx._h, f.ctypes.data_as(dp), 1, 96, 120, C.byref(p), 0, C.byref(n),
                                                 off.ctypes.data_as(lp), g.ctypes.data_as(dp), *([None] * 11), wstruct, None)

    wp = weights.ctypes.data_as(dp)
    assert call(1.5, None) == -1
    assert call(1.5, C.byref(_lib.DvDetectWeights(None, 0, 0))) == -1
    assert call(1.5, C.byref(_lib.DvDetectWeights(wp, 2, 0))) == -1
    assert call(1.5, C.byref(_lib.DvDetectWeights(wp, 0, -1))) == -1
    assert call(0.0, C.byref(_lib.DvDetectWeights(wp, 0, 0))) == -1
    assert "sigma" in _lib.last_error()
    assert call(1.5, C.byref(_lib.DvDetectWeights(wp, 1, 0))) == 0 and n.value == len(ref["x"])
    with pytest.raises(ValueError):
        ctx.scene_detect(data[None], weights=weights[None], thresh=0.0)
    with pytest.raises(ValueError, match="counts"):
        ctx.scene_detect(data[None], weights=np.ones_like(weights)[None])          # NaN under a counting pixel
    with pytest.raises(ValueError, match="weighted call"):
        ctx.scene_detect(f, filter_type="matched")
    with pytest.raises(DvError):
        ctx.scene_detect(data[None], weights=weights[None], workspace_bytes=1)
    _same_bits(ref, ctx.scene_detect(data[None], weights=weights[None], back_size=32))


def test_field_without_a_good_mesh_between_two_others():
    fields, w = _three()
    w[1] = 0.0
    w[1, 40:60, 40:52] = 1.0                            # 240 counting pixels: under half of the mesh they lie in
    fields[1, :30] = np.nan
    ctx = _ctx()
    for kw in SETTINGS:
        got = ctx.scene_detect(fields, weights=w, return_maps=True, back_size=32, **kw)
        assert got["offsets"][1] == got["offsets"][2] and np.isnan(got["globalrms"][1])
        assert (got["labels"][1] == -1).all() and got["bad_meshes"].tolist() == [1, 12, 1]
        assert not (got["field"] == 1).any()
        for i in (0, 2):
            one = ctx.scene_detect(fields[i:i + 1], weights=w[i:i + 1], return_maps=True, back_size=32, **kw)
            lo, hi = got["offsets"][i], got["offsets"][i + 1]
            assert hi - lo == len(one["x"]) > 0
            for k in CAT[1:]:
                np.testing.assert_array_equal(one[k], got[k][lo:hi], err_msg=k)
            for k in MAPS:
                np.testing.assert_array_equal(one[k][0], got[k][i], err_msg=k)
            assert one["globalrms"][0] == got["globalrms"][i]


def _set_case():
    from tests.test_gpu_fields_batch import _blob_fields

    F = 131
    fields = _blob_fields(4, F, seed=11)
    rng = np.random.default_rng(12)
    w = rng.uniform(200.0, 600.0, (4, F, F))            # inverse variances around the fields' noise of 0.05
    w[:, :, 66] = 0.0
    w[2, 20:50, 20:60] = np.nan
    return fields, w


def test_field_set_detects_with_the_planes_it_holds():
    from debvader_amd import _lib
    from debvader_amd._lib import DvError
    from tests.test_gpu_fields_batch import _case, _net

    net = _net("float32")
    ctx, eng = net._core.ctx, net._core.engine
    fields, w = _set_case()
    F = fields.shape[1]
    starts, places, fp = _case(F, [12, 0, 30, 7], seed=5, hang=False)
    fs = eng.open_field_set(fields)
    fs.deblend_pass(starts, places, fp, seed=3)
    work = fs.read("work")
    plain = fs.detect()
    for noise, filt, thresh in (("absolute", "conv", 1.5), ("absolute", "matched", 4.0), ("relative", "conv", 1.5)):
        fs.set_detect_weights(w, noise=noise, filter_type=filt)
        for active in (None, np.array([True, False, True, True])):
            got = fs.detect(active=active, thresh=thresh, back_size=32)
            on = np.ones(4, bool) if active is None else active
            ref = ctx.scene_detect(work[on][:, :, :, 2], weights=w[on], noise=noise, filter_type=filt, thresh=thresh,
                                   back_size=32)
            idx = np.nonzero(on)[0]
            counts = np.zeros(4, np.int64)
            counts[idx] = np.diff(ref["offsets"])
            np.testing.assert_array_equal(got["offsets"], np.concatenate([[0], np.cumsum(counts)]))
            assert len(ref["x"]) > 0
            _same_bits(ref, got, CAT[1:])
            np.testing.assert_array_equal(got["field"], idx[ref["field"]])
            np.testing.assert_array_equal(got["globalrms"][on], ref["globalrms"])
            assert not got["globalrms"][~on].any()
    # four-dimensional weights: band 2 (and noise "absolute" by default, which refuses thresh <= 0)
    w4 = np.repeat(np.ones_like(w)[..., None], 6, axis=3)
    w4[..., 2] = w
    fs.set_detect_weights(w4)
    got = fs.detect(back_size=32)
    _same_bits(ctx.scene_detect(work[:, :, :, 2], weights=w, back_size=32), got, CAT[1:])
    with pytest.raises(ValueError):
        fs.detect(thresh=0.0)
    with pytest.raises(ValueError):
        fs.set_detect_weights(w[:, :100])
    with pytest.raises(ValueError):
        fs.set_detect_weights(w, noise="poisson")
    _same_bits(got, fs.detect(back_size=32))
    # dropped: the unweighted bits
    fs.set_detect_weights(None)
    _same_bits(plain, fs.detect())
    fs.set_detect_weights(w)
    raw = C.c_void_p(fs._h.value)
    fs.close()
    with pytest.raises(DvError, match="closed"):
        fs.set_detect_weights(w)
    wc = np.ascontiguousarray(w)
    assert _lib.lib.dv_field_set_detect_weights(raw, wc.ctypes.data_as(C.POINTER(C.c_double)), 0, 0) == -5
    assert _lib.lib.dv_field_set_detect_weights(raw, None, 0, 0) == -5


def _loop_case():
    """two 119-px fields with a bleed column at column 70, filled with a finite value, and the weights that mask it"""
    from tests.test_gpu_fields_batch import NB

    F = 119
    rng = np.random.default_rng(31)
    fields = rng.normal(0, 0.05, (2, F, F, NB))
    yy, xx = np.mgrid[:F, :F]
    for m, blobs in enumerate((((40, 45, 2.0, 6.0), (75, 50, 2.5, 8.0), (60, 88, 2.0, 5.0)),
                               ((50, 40, 2.0, 7.0), (80, 90, 3.0, 9.0)))):
        for r, c, s, a in blobs:
            fields[m] += (a * np.exp(-0.5 * ((yy - r) ** 2 + (xx - c) ** 2) / s ** 2))[:, :, None]
    fields[:, :, 70, :] = 40.0
    w = np.full((2, F, F), 1.0 / 0.05 ** 2)
    w[:, :, 70] = 0.0
    return fields, w


def _on_column(rec, F=119, col=70):
    """rows whose detection lies on the column: the rounded barycentre is the column's.  (No component of the weighted
    detector crosses the column, where S = -inf, so none of them is centred on it.)"""
    return int(F / 2) + np.asarray(rec["galaxy_distances_to_center_y"], dtype=np.float64) == col


def test_iterative_catalogue_with_detect_weights():
    from debvader_amd.deblend.field_deblender import batch_windows
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch
    from debvader_amd.detect.detection import _distances
    from tests.test_gpu_fields_batch import CS, NB
    from tests.test_gpu_iterative_batch import _loop_net

    fields, w = _loop_case()
    F = fields.shape[1]
    net = _loop_net("float32")

    def loop():                                         # (the seed counter of a net starts at a random number)
        net._core.seed_counter = 500
        return IterativeDeblendFieldBatch(net, fields, CS, NB)

    it = loop()
    res = it.iterative_catalogue(detect_weights=w)
    # pass 0: the oracle's detections on the fields as given
    dist = []
    for m in range(2):
        c = wo.detect(fields[m, :, :, 2], w[m])
        assert len(c["x"]) == it.nb_of_detected_objects[0][m] > 0
        dist.append(_distances(c["x"], c["y"], F))
    _, fp, kept, dd = batch_windows(F, dist, CS)
    for m in range(2):
        first = res[m][res[m]["iteration"] == 0]
        np.testing.assert_array_equal(first["list_idx"], kept[m])
        np.testing.assert_array_equal(first["galaxy_distances_to_center_x"], dd[fp[m]:fp[m + 1], 0])
        np.testing.assert_array_equal(first["galaxy_distances_to_center_y"], dd[fp[m]:fp[m + 1], 1])
        assert len(res[m]) > 0 and not _on_column(res[m]).any()
    # the same call without weights detects the column
    plain = loop()
    a = plain.iterative_catalogue(detect_weights=None)
    assert all(_on_column(r).any() for r in a)
    # ... and is the call as it was: the bits of iterative_deblending()
    old = loop()
    b = old.iterative_deblending()
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and len(x) == len(y)
        for name in x.dtype.names:
            assert all(np.array_equal(p, q, equal_nan=True) for p, q in zip(x[name], y[name])), name
    assert plain.mse == old.mse
    np.testing.assert_array_equal(plain.get_residual_fields(), old.get_residual_fields())
