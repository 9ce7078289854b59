"""The GPU source detector on the inverse-variance combination of several bands (Context.scene_detect_multiband,
dv_scene_detect_multiband, FieldSet.set_detect_bands) against its numpy restatement
(tests/detect_multiband_oracle.py), against the single-band detector where the section promises its bits, and through the
resident set and the iterative loop.  Tolerances against the oracle are those of tests/test_gpu_detect.py."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

from tests import detect_multiband_oracle as mo

pytestmark = pytest.mark.gpu

CAT = ("field", "parent", "npix", "peak", "flux", "x", "y")
MAPS = ("back", "rms", "V", "Wt", "D", "labels")
KW = dict(thresh=mo.THRESH, back_size=mo.BACK_SIZE)


def _ctx():
    from debvader_amd import engine as E
    return E.default_context()


def _compare(got, i, exp):
    """field i of a scene_detect_multiband result with maps against the oracle's detect() of the same field; prints the
    fraction of every bound that is used"""
    for k in ("back", "rms", "V", "Wt", "D"):
        g, e = got[k][i], exp[k]
        np.testing.assert_array_equal(np.isneginf(g), np.isneginf(e), err_msg=k)
        np.testing.assert_array_equal(np.isnan(g), np.isnan(e), err_msg=k)
        fin = np.isfinite(e)
        assert np.isfinite(g[fin]).all() and not np.isposinf(g).any(), k
        if not fin.any():
            continue
        scale = np.abs(e[fin]).max()
        err = np.abs(g[fin] - e[fin]).max()
        print(f"{k}: max error {err:.3e}, bound {1e-12 * scale:.3e}, fraction {err / max(1e-12 * scale, 1e-300):.3f}")
        assert err <= 1e-12 * scale, k
    for k in ("globalrms", "band_globalrms"):
        np.testing.assert_allclose(got[k][i], exp[k], rtol=1e-12, atol=0, err_msg=k)
    np.testing.assert_array_equal(got["labels"][i], exp["labels"])
    np.testing.assert_array_equal(got["bad_meshes"][i], exp["bad_meshes"])
    lo, hi = got["offsets"][i], got["offsets"][i + 1]
    assert hi - lo == len(exp["x"]), (hi - lo, len(exp["x"]))
    assert (got["field"][lo:hi] == i).all()
    np.testing.assert_array_equal(got["npix"][lo:hi], exp["npix"])
    np.testing.assert_array_equal(got["parent"][lo:hi], exp["parent"])
    for k in ("peak", "flux"):
        scale = max(np.abs(exp[k]).max(), 1e-300) if len(exp[k]) else 1.0
        if len(exp[k]):
            print(f"{k}: fraction {np.abs(got[k][lo:hi] - exp[k]).max() / (1e-12 * scale):.3f}")
        np.testing.assert_allclose(got[k][lo:hi], exp[k], rtol=0, atol=1e-12 * scale, err_msg=k)
    for k in ("x", "y"):
        if len(exp[k]):
            print(f"{k}: fraction {np.abs(got[k][lo:hi] - exp[k]).max() / 1e-9:.3e}")
        np.testing.assert_allclose(got[k][lo:hi], exp[k], rtol=0, atol=1e-9, err_msg=k)


def _same_bits(a, b, keys=None):
    for k in keys or a:
        assert k in b, k
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        assert a[k].dtype == b[k].dtype, k


def _defects():
    """the scene with a stripe masked in every band and a block masked in band 3 only, NaN under both; (fields, planes
    (inverse variances), mask (H, W, 6), positions)"""
    fields, pos = mo.scene()
    P = mo.variance_planes()
    mask = np.zeros(fields.shape, bool)
    mask[:, 52, :] = True
    mask[10:14, 60:70, 3] = True
    fields = fields.copy()
    fields[mask] = np.nan
    P[mask] = 0.0
    return fields, P, mask, pos


SETTINGS = {"plain-conv": dict(filter_type="conv", **KW),
            "absolute-conv": dict(filter_type="conv", noise="absolute", **KW),
            "absolute-matched": dict(filter_type="matched", noise="absolute", thresh=6.0, back_size=mo.BACK_SIZE),
            "mask-only": dict(filter_type="conv", **KW)}


@pytest.mark.parametrize("name", list(SETTINGS))
def test_scene_stage_by_stage(name):
    kw = SETTINGS[name]
    fields, P, mask, pos = _defects()
    if name == "plain-conv":
        fields, pos = mo.scene()
        got = _ctx().scene_detect_multiband(fields[None], return_maps=True, **kw)
        exp = mo.detect(fields, **kw)
    elif name == "mask-only":
        got = _ctx().scene_detect_multiband(fields[None], mask=mask[None], return_maps=True, **kw)
        exp = mo.detect(fields, planes=np.where(mask, 0.0, 1.0), noise="relative", **kw)
    else:
        got = _ctx().scene_detect_multiband(fields[None], weights=P[None], return_maps=True, **kw)
        exp = mo.detect(fields, planes=P, **kw)
    assert np.abs(exp["D"][np.isfinite(exp["D"])] - kw["thresh"]).min() > 1e-9      # no label sits on a rounding edge
    _compare(got, 0, exp)
    d = np.hypot(np.array([pos[n][0] for n in ("all", "r_only", "not_r", "faint")])[:, None] - got["y"][None],
                 np.array([pos[n][1] for n in ("all", "r_only", "not_r", "faint")])[:, None] - got["x"][None])
    assert (d.min(axis=1) <= 1.0).all()
    if name != "plain-conv":
        assert np.isneginf(got["D"][0][:, 52]).all() and np.isfinite(got["D"][0][10:14, 60:70]).all()
    if name == "plain-conv":
        assert len(exp["x"]) == 4                       # "red" stays under the threshold
        # the single band of the reference's sep call finds two of them
        r = _ctx().scene_detect(fields[None, :, :, 2], thresh=1.5, back_size=mo.BACK_SIZE)
        near = lambda n: (np.hypot(r["y"] - pos[n][0], r["x"] - pos[n][1]) <= 2.0).any()
        assert near("all") and near("r_only") and not near("not_r")


def _small():
    rng = np.random.default_rng(6)
    y, x = np.mgrid[:40, :50]
    g = lambda cy, cx, s, a: a * np.exp(-0.5 * ((x - cx) ** 2 + (y - cy) ** 2) / s ** 2)
    f = np.stack([3.0 + rng.normal(0, 2.0, (40, 50)), 7.0 + rng.normal(0, 1.0, (40, 50)), -2.0 + rng.normal(0, 0.5, (40, 50))],
                 axis=-1)
    f[:, :, 0] += g(20, 25, 2.0, 30.0) + g(8, 40, 1.5, 25.0)
    f[:, :, 2] += g(20, 25, 2.0, 10.0) + g(30, 10, 1.5, 6.0)
    return f


def test_field_smaller_than_one_mesh_with_a_non_square_kernel_and_two_of_three_bands():
    f = _small()
    kern = np.outer([1.0, 2.0, 1.0], [1.0, 3.0, 4.0, 3.0, 1.0])
    kw = dict(bands=(2, 0), band_weights=(1.0, 0.5), filter_kernel=kern, thresh=2.5)
    got = _ctx().scene_detect_multiband(f[None], return_maps=True, **kw)
    exp = mo.detect(f, **kw)
    assert len(exp["x"]) >= 2 and np.abs(exp["D"] - 2.5).min() > 1e-9
    _compare(got, 0, exp)
    P = np.full((40, 50, 2), 0.25)
    P[:, 30, :] = 0.0
    P[12, :8, 1] = np.nan
    f[12, :8, 0] = np.nan
    for filt in ("conv", "matched"):
        got = _ctx().scene_detect_multiband(f[None], weights=P[None], noise="relative", filter_type=filt, return_maps=True, **kw)
        _compare(got, 0, mo.detect(f, planes=P, noise="relative", filter_type=filt, **kw))


@functools.lru_cache(maxsize=None)
def _three():
    a, _ = mo.scene()
    b, _ = mo.scene(seed=12)
    fields = np.stack([a, b[::-1], a[:, ::-1]])
    fields.setflags(write=False)
    return fields, _ctx().scene_detect_multiband(fields, return_maps=True, **KW)


def test_bands_have_the_bits_of_the_single_band_detector():
    fields, ref = _three()
    ctx = _ctx()
    for j in (0, 5):
        one = ctx.scene_detect(np.ascontiguousarray(fields[:, :, :, j]), return_maps=True, back_size=mo.BACK_SIZE)
        np.testing.assert_array_equal(ref["back"][..., j], one["back"])
        np.testing.assert_array_equal(ref["rms"][..., j], one["rms"])
        np.testing.assert_array_equal(ref["band_globalrms"][:, j], one["globalrms"])
    assert not ref["bad_meshes"].any()
    # k = 1: the weighted single-band call on 1 / rms^2 of its own maps, every output
    band = np.ascontiguousarray(fields[:, :, :, 2])
    k1 = ctx.scene_detect_multiband(fields, bands=[2], return_maps=True, **KW)
    rms = k1["rms"][..., 0]
    w = 1.0 / (rms * rms)
    single = ctx.scene_detect(band, weights=w, noise="absolute", return_maps=True, **KW)
    assert len(single["x"]) >= 3
    _same_bits(single, k1, CAT + ("offsets", "D", "labels"))
    np.testing.assert_array_equal(k1["Wt"], w)
    np.testing.assert_array_equal(k1["back"][..., 0], single["back"])
    np.testing.assert_array_equal(k1["rms"][..., 0], single["rms"])
    np.testing.assert_array_equal(k1["V"], band - single["back"])
    np.testing.assert_array_equal(k1["band_globalrms"][:, 0], single["globalrms"])
    # unit relative planes: the call without planes
    _same_bits(ref, ctx.scene_detect_multiband(fields, weights=np.ones(fields.shape), noise="relative", return_maps=True, **KW))
    _same_bits(ref, ctx.scene_detect_multiband(fields, mask=np.zeros(fields.shape[:3], bool), return_maps=True, **KW))
    # a selection in another order: the same planes, the sums in that order
    rev = ctx.scene_detect_multiband(fields, bands=[5, 4, 3, 2, 1, 0], return_maps=True, **KW)
    np.testing.assert_array_equal(rev["back"], ref["back"][..., ::-1])
    np.testing.assert_array_equal(rev["band_globalrms"], ref["band_globalrms"][:, ::-1])
    np.testing.assert_allclose(rev["Wt"], ref["Wt"], rtol=1e-14)
    assert len(rev["x"]) == len(ref["x"])


def _need(msg):
    m = re.search(r"needs up to (\d+) bytes", msg)
    assert m, msg
    return int(m.group(1))


def test_bit_reproducible_independent_of_the_batch_and_of_the_workspace():
    from debvader_amd._lib import DvError

    fields, a = _three()
    ctx = _ctx()
    kw = dict(return_maps=True, **KW)
    assert (np.diff(a["offsets"]) > 0).all()
    _same_bits(a, ctx.scene_detect_multiband(fields, **kw))
    for i in range(3):
        one = ctx.scene_detect_multiband(fields[i:i + 1], **kw)
        lo, hi = a["offsets"][i], a["offsets"][i + 1]
        for k in CAT[1:]:
            np.testing.assert_array_equal(one[k], a[k][lo:hi], err_msg=k)
        for k in MAPS + ("globalrms", "band_globalrms", "bad_meshes"):
            np.testing.assert_array_equal(one[k][0], a[k][i], err_msg=k)
    # what one field needs, as the refusal names it: the planes, the k-fold grids and splines and Wt are counted
    with pytest.raises(DvError, match="workspace") as six:
        ctx.scene_detect_multiband(fields, workspace_bytes=1, **kw)
    with pytest.raises(DvError, match="workspace") as two:
        ctx.scene_detect_multiband(fields, bands=[0, 1], workspace_bytes=1, **kw)
    with pytest.raises(DvError, match="workspace") as planes:
        ctx.scene_detect_multiband(fields, weights=np.ones(fields.shape), workspace_bytes=1, **kw)
    need = _need(str(six.value))
    HW, H, ny, nx = 96 * 120, 96, 3, 4
    per_band = HW * 8 * 3 + H * nx * 4 * 8 + ny * nx * 6 * 8 + 12            # the data plane, back and rms maps, splines, grids
    assert need - _need(str(two.value)) == 4 * per_band
    assert _need(str(planes.value)) - need == 6 * HW * 8
    c = ctx.scene_detect_multiband(fields, workspace_bytes=need, **kw)       # one field per launch
    _same_bits(a, c)
    with pytest.raises(DvError, match="workspace") as below:
        ctx.scene_detect_multiband(fields, workspace_bytes=need - 1, **kw)
    assert _need(str(below.value)) == need
    _same_bits(a, ctx.scene_detect_multiband(fields, **kw))


@pytest.mark.parametrize("with_planes", [False, True])
def test_one_field_per_launch_gives_the_same_bytes_with_two_of_three_bands(with_planes):
    """three 48 x 40 fields of three bands on 3 x 3 meshes of 16 px, bands 2 and 0 selected in that order, a few sources
    each: the default workspace (one launch) against a workspace that holds exactly one field (three launches), every
    output - the [..][k] maps, band_globalrms and bad_meshes at field * k among them"""
    from debvader_amd._lib import DvError

    rng = np.random.default_rng(22)
    y, x = np.mgrid[:48, :40]
    fields = np.array([4.0, -1.0, 9.0]) + rng.normal(0, 1.0, (3, 48, 40, 3)) * np.array([1.0, 3.0, 0.5])
    for i, srcs in enumerate((((12, 10), (30, 28), (40, 8)), ((8, 30), (24, 20)), ((20, 12), (36, 30), (10, 34)))):
        for cy, cx in srcs:
            g = np.exp(-0.5 * ((x - cx) ** 2 + (y - cy) ** 2) / 1.8 ** 2)
            fields[i] += g[:, :, None] * np.array([30.0, 5.0, 12.0])
    kw = dict(bands=[2, 0], band_weights=[1.0, 0.5], thresh=3.0, back_size=16, return_maps=True)
    if with_planes:
        P = rng.uniform(0.5, 2.0, (3, 48, 40, 2))
        P[1, :, 17, :] = 0.0                              # a masked column in field 1, a bad mesh in band 2 of field 2
        P[2, 32:, 24:, 0] = 0.0
        kw.update(weights=P, noise="absolute")
    ctx = _ctx()
    a = ctx.scene_detect_multiband(fields, **kw)
    assert (np.diff(a["offsets"]) >= 2).all()
    if with_planes:
        assert a["bad_meshes"].tolist() == [[0, 0], [0, 0], [1, 0]]
    with pytest.raises(DvError, match="workspace") as refused:
        ctx.scene_detect_multiband(fields, **dict(kw, workspace_bytes=1))
    b = ctx.scene_detect_multiband(fields, **dict(kw, workspace_bytes=_need(str(refused.value))))
    assert set(a) == set(b) and set(MAPS) <= set(a)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


def test_values_under_bands_that_do_not_count_reach_no_sum():
    fields, P, mask, _ = _defects()
    ctx = _ctx()
    for kw in (SETTINGS["absolute-conv"], SETTINGS["absolute-matched"]):
        ref = ctx.scene_detect_multiband(fields[None], weights=P[None], return_maps=True, **kw)
        assert len(ref["x"]) >= 4
        for val in (np.inf, -np.inf, 1e300, 0.0):
            d = fields.copy()
            d[mask] = val
            _same_bits(ref, ctx.scene_detect_multiband(d[None], weights=P[None], return_maps=True, **kw))


def test_a_band_and_a_field_without_a_good_mesh():
    fields, _ = _three()
    fields = fields.copy()
    ctx = _ctx()
    P = np.broadcast_to(mo.variance_planes(), fields.shape).copy()
    P[1] = 0.0                                          # field 1: no band has a good mesh
    P[1, 40:60, 40:52, :] = 1.0
    fields[1, :30] = np.nan
    P[2, :, :, 5] = 0.0                                 # field 2: band 5 has none
    fields[2, :, :, 5] = np.nan
    got = ctx.scene_detect_multiband(fields, weights=P, return_maps=True, **KW)
    assert got["offsets"][1] == got["offsets"][2] and np.isnan(got["globalrms"][1]) and (got["labels"][1] == -1).all()
    assert got["bad_meshes"].tolist() == [[0] * 6, [12] * 6, [0] * 5 + [12]] and np.isnan(got["band_globalrms"][2, 5])
    assert np.isneginf(got["D"][1]).all() and not got["V"][1].any() and not got["Wt"][1].any()
    for i in (0, 2):
        _compare(got, i, mo.detect(fields[i], planes=P[i], noise="absolute", **KW))
    five = ctx.scene_detect_multiband(fields[2:3], bands=range(5), weights=P[2:3, :, :, :5], return_maps=True, **KW)
    for k in ("V", "Wt", "D", "labels"):
        np.testing.assert_array_equal(five[k][0], got[k][2], err_msg=k)


def test_refusals_leave_the_engine_usable():
    from debvader_amd import _lib
    from debvader_amd._lib import DvError

    fields, ref = _three()
    ctx = _ctx()
    f = np.ascontiguousarray(fields[:1])
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    n, off, g = C.c_int64(), np.zeros(2, np.int64), np.zeros(1)
    ones = np.ones(6)

    def call(bands, cw=None, planes=None, noise=0, filt=0, thresh=mo.THRESH, nb=6, struct=True):
        b = np.asarray(bands, np.int32)
        p = _lib.DvDetectParams(thresh, 1e-5, 4, 64, mo.BACK_SIZE, 3, None, 0, 0, 0)
        s = _lib.DvDetectBands(b.ctypes.data_as(ip), len(b), None if cw is None else np.asarray(cw, float).ctypes.data_as(dp),
                               None if planes is None else planes.ctypes.data_as(dp), noise, filt)
        return _lib.lib.dv_scene_detect_multiband(ctx._h, f.ctypes.data_as(dp), 1, 96, 120, nb, C.byref(p), 0, C.byref(n),
                                                  off.ctypes.data_as(lp), g.ctypes.data_as(dp), *([None] * 13),
                                                  C.byref(s) if struct else None, None, None)

    P = np.ones(f.shape)
    assert call(range(6), struct=False) == -1
    assert call([]) == -1 and call(list(range(6)) + [0]) == -1                   # k < 1, k > nb
    assert call([6]) == -1 and call([-1]) == -1 and call([1, 1]) == -1
    assert "twice" in _lib.last_error()
    for bad in (0.0, -1.0, np.inf, np.nan):
        assert call([0, 1], cw=[1.0, bad]) == -1
    assert call(range(6), planes=P, noise=2) == -1 and call(range(6), filt=2) == -1
    assert call(range(6), thresh=0.0) == -1 and call(range(6), planes=P, noise=1, thresh=-1.0) == -1
    assert "sigma" in _lib.last_error()
    assert call(range(3), nb=0) == -1
    assert call(range(6), cw=ones) == 0 and n.value == ref["offsets"][1]
    with pytest.raises(ValueError):
        ctx.scene_detect_multiband(fields, bands=[0, 0])
    with pytest.raises(ValueError):
        ctx.scene_detect_multiband(fields, thresh=0.0)
    with pytest.raises(DvError):
        ctx.scene_detect_multiband(fields, workspace_bytes=1)
    _same_bits(ref, ctx.scene_detect_multiband(fields, return_maps=True, **KW))


def test_field_set_detects_with_the_selection_it_holds():
    from debvader_amd import _lib
    from debvader_amd._lib import DvError
    from tests.test_gpu_fields_batch import _blob_fields, _case, _net

    net = _net("float32")
    ctx, eng = net._core.ctx, net._core.engine
    F = 131
    fields = _blob_fields(2, F, seed=11)
    rng = np.random.default_rng(12)
    w = rng.uniform(200.0, 600.0, (2, F, F, 6))         # inverse variances around the fields' noise of 0.05
    w[:, :, 66, :] = 0.0
    w[1, 20:50, 20:60, 4] = np.nan
    starts, places, fp = _case(F, [12, 7], seed=5, hang=False)
    fs = eng.open_field_set(fields)
    fs.deblend_pass(starts, places, fp, seed=3)
    work = fs.read("work")
    plain = fs.detect()

    def check(got, ref, on):
        idx = np.nonzero(on)[0]
        counts = np.zeros(2, np.int64)
        counts[idx] = np.diff(ref["offsets"])
        np.testing.assert_array_equal(got["offsets"], np.concatenate([[0], np.cumsum(counts)]))
        assert len(ref["x"]) > 0
        _same_bits(ref, got, CAT[1:])
        np.testing.assert_array_equal(got["field"], idx[ref["field"]])
        np.testing.assert_array_equal(got["globalrms"][on], ref["globalrms"])
        assert not got["globalrms"][~on].any()

    for sel, cw, planes, noise, filt, thresh in ((None, None, None, None, "conv", 2.5), ((4, 1, 2), (1.0, 0.5, 2.0), None, None,
                                                                                          "matched", 5.0),
                                                 (range(6), None, w, "absolute", "conv", 2.5), ((5, 0), None, w[..., [5, 0]],
                                                                                                "relative", "matched", 5.0)):
        fs.set_detect_bands(range(6) if sel is None else sel, band_weights=cw, weights=planes, noise=noise, filter_type=filt)
        for active in (None, np.array([False, True])):
            got = fs.detect(active=active, thresh=thresh, back_size=32)
            on = np.ones(2, bool) if active is None else active
            ref = ctx.scene_detect_multiband(work[on], bands=sel, band_weights=cw, weights=None if planes is None else planes[on],
                                             noise=noise, filter_type=filt, thresh=thresh, back_size=32)
            check(got, ref, on)
    with pytest.raises(ValueError):
        fs.detect(thresh=0.0)
    with pytest.raises(ValueError):
        fs.set_detect_bands([0, 0])
    with pytest.raises(ValueError):
        fs.set_detect_bands([0, 1], weights=w)
    with pytest.raises(DvError, match="band selection"):
        fs.set_detect_weights(w[..., 2])
    _same_bits(got, fs.detect(active=np.array([False, True]), thresh=5.0, back_size=32))
    # dropped: band 2 alone, the bits of before; single-band planes then refuse a selection
    fs.set_detect_bands(None)
    _same_bits(plain, fs.detect())
    fs.set_detect_weights(w[..., 2])
    with pytest.raises(DvError, match="single-band planes"):
        fs.set_detect_bands(range(6))
    fs.set_detect_weights(None)
    fs.set_detect_bands([2])
    raw = C.c_void_p(fs._h.value)
    fs.close()
    with pytest.raises(DvError, match="closed"):
        fs.set_detect_bands([2])
    assert _lib.lib.dv_field_set_detect_bands(raw, None, 0, None, None, 0, 0) == -5


def test_iterative_catalogue_with_detect_bands():
    from debvader_amd.deblend.field_deblender import batch_windows
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch
    from debvader_amd.detect.detection import _distances
    from tests.test_gpu_detect_weighted import _loop_case
    from tests.test_gpu_fields_batch import CS, NB
    from tests.test_gpu_iterative_batch import _loop_net

    fields, w = _loop_case()
    fields[:, :, 70, :] = fields[:, :, 69, :]            # (no bleed column here: the fields as they would be without one)
    F = fields.shape[1]
    net = _loop_net("float32")
    net._core.seed_counter = 500
    it = IterativeDeblendFieldBatch(net, fields, CS, NB)
    res = it.iterative_catalogue(detect_bands=range(6), detect_thresh=3.0)
    first = net._core.ctx.scene_detect_multiband(fields, thresh=3.0)
    off = first["offsets"]
    dist = [_distances(first["x"][off[m]:off[m + 1]], first["y"][off[m]:off[m + 1]], F) for m in range(2)]
    assert [len(d) for d in dist] == it.nb_of_detected_objects[0] and min(len(d) for d in dist) > 0
    _, fp, kept, dd = batch_windows(F, dist, CS)
    for m in range(2):
        one = res[m][res[m]["iteration"] == 0]
        np.testing.assert_array_equal(one["list_idx"], kept[m])
        np.testing.assert_array_equal(one["galaxy_distances_to_center_x"], dd[fp[m]:fp[m + 1], 0])
        np.testing.assert_array_equal(one["galaxy_distances_to_center_y"], dd[fp[m]:fp[m + 1], 1])
        assert len(res[m]) > 0
