"""The detector's object columns and segmentation map on the GPU (Context.scene_detect_objects, dv_scene_detect_objects,
FieldSet.set_detect_objects) against their numpy restatement (tests/detect_objects_oracle.py): on the
painted fields of tests/detect_shapes.py, where every set membership is exact, on the two noisy scenes with defects, across
the chunks of a batch, through the resident set and the iterative loop.  Every shared output has the bits of the existing
call on the same input.  The fraction of every bound met is printed (DESIGN.md quotes the worst)."""
import ctypes as C

import numpy as np
import pytest

from tests import detect_multiband_oracle as mo
from tests import detect_objects_oracle as oo
from tests import detect_shapes as ds
from tests import detect_weighted_oracle as wo

pytestmark = pytest.mark.gpu

CAT = ("field", "parent", "npix", "peak", "flux", "x", "y")
SHARED = CAT + ("offsets", "globalrms")
INT = oo.INT_KEYS
DBL = oo.DOUBLE_KEYS
DERIVED = ("a", "b", "theta", "cxx", "cyy", "cxy")


def _ctx():
    from debvader_amd import engine as E
    return E.default_context()


def _same_bits(a, b, keys):
    for k in keys:
        assert a[k].dtype == b[k].dtype, k
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def _compare(got, i, exp, obj, v):
    """field i of a scene_detect_objects result with a segmap against the restatement's objects of that field; v is the map
    flux sums as the GPU computed it (the bits of vpeak are its bits there; the restatement's v agrees to 1e-12 of its scale)"""
    lo, hi = got["offsets"][i], got["offsets"][i + 1]
    assert hi - lo == len(obj["npix"]) == len(exp["x"])
    np.testing.assert_array_equal(got["segmap"][i], obj["segmap"])
    np.testing.assert_array_equal(got["npix"][lo:hi], obj["npix"])
    for k in INT:
        np.testing.assert_array_equal(got[k][lo:hi], obj[k], err_msg=k)
    np.testing.assert_array_equal(got["vpeak"][lo:hi], v[got["yvpeak"][lo:hi], got["xvpeak"][lo:hi]])
    np.testing.assert_allclose(got["vpeak"][lo:hi], obj["vpeak"], rtol=0, atol=1e-12 * max(np.abs(exp["v" if "v" in exp else "V"]).max(), 1e-300))
    if hi == lo:
        return
    frac = {}
    err = np.abs(got["dflux"][lo:hi] - obj["dflux"])
    frac["dflux"] = (err / (1e-12 * np.abs(obj["dflux"]))).max()           # (D > T >= 0: sum |D| is dflux)
    for k in ("x_iso", "y_iso"):
        frac[k] = (np.abs(got[k][lo:hi] - obj[k]) / 1e-9).max()
    bound = 1e-9 * np.maximum(1.0, obj["x2"] + obj["y2"])
    for k in ("x2", "y2", "xy"):
        frac[k] = (np.abs(got[k][lo:hi] - obj[k]) / bound).max()
    print("fraction of the bound met:", ", ".join(f"{k} {f:.2e}" for k, f in frac.items()))
    for k, f in frac.items():
        assert f <= 1.0, (k, f)
    d = oo.derived(got["x2"][lo:hi], got["y2"][lo:hi], got["xy"][lo:hi])
    for k in DERIVED:
        np.testing.assert_allclose(got[k][lo:hi], d[k], rtol=1e-13, atol=1e-13, err_msg=k)


def _objects_of(name, path):
    data, exp, details, kw = ds.oracle(name, path)
    facts = ds.CASES[name]()[2]
    ds.check_premises(data, exp, details, kw)                 # P1 - P4
    ds.check_facts(data, exp, details, facts)                 # P5
    obj = oo.objects(details, exp["D"], exp["v"], wt=np.ones_like(data) if path == "weighted" else None)
    return data, exp, obj, kw


@pytest.mark.parametrize("name", list(ds.CASES))
def test_painted_fields_weighted_path(name):
    data, exp, obj, kw = _objects_of(name, "weighted")
    w = np.ones_like(data)[None]
    got = _ctx().scene_detect_objects(data[None], weights=w, segmentation_map=True, **kw)
    _same_bits(got, _ctx().scene_detect(data[None], weights=w, **kw), SHARED)
    _compare(got, 0, exp, obj, exp["v"])
    assert not (got["flag"] & 8).any()


@pytest.mark.parametrize("name", list(ds.UNWEIGHTED))
def test_painted_fields_unweighted_path(name):
    data, exp, obj, kw = _objects_of(name, "unweighted")
    got = _ctx().scene_detect_objects(data[None], segmentation_map=True, **kw)
    _same_bits(got, _ctx().scene_detect(data[None], **kw), SHARED)
    _compare(got, 0, exp, obj, exp["v"])
    assert not (got["flag"] & 8).any()


def _v(data, back, w):
    """the v map of the weighted call from the back map it returns: data - back where the pixel counts, 0 elsewhere"""
    v = np.zeros_like(data)
    on = oo.counting(w)
    v[on] = data[on] - back[on]
    return v


def test_weighted_scene_with_defects():
    """the scene's own seed 11 holds P3 / P4 on the restatement with the conv filter and with the mask alone; with the matched
    filter it does not (a pixel of the component at 8497 lies 1.1e-4 from a level, P = 4e2) and seed 12 is the first that does"""
    data, weights, mask, _ = wo.scene()
    for seed, kw in ((11, dict(filter_type="conv", noise="absolute", thresh=1.5)),
                     (12, dict(filter_type="matched", noise="absolute", thresh=5.0))):
        data, weights, mask, _ = wo.scene(seed=seed)
        exp, obj, details = oo.detect_weighted(data, weights, back_size=32, **kw)
        oo.check_p3_p4(details)
        assert (obj["flag"] & oo.MASKED).any() and not (obj["flag"] & oo.MASKED).all()
        got = _ctx().scene_detect_objects(data[None], weights=weights[None], back_size=32, segmentation_map=True, **kw)
        ref = _ctx().scene_detect(data[None], weights=weights[None], back_size=32, return_maps=True, **kw)
        _same_bits(got, ref, SHARED)
        _compare(got, 0, exp, obj, _v(data, ref["back"][0], weights))
    # the mask alone, through mask=: relative weights (seed 11)
    data, weights, mask, _ = wo.scene()
    exp, obj, details = oo.detect_weighted(data, np.where(mask, 0.0, 1.0), noise="relative", back_size=32)
    oo.check_p3_p4(details)
    got = _ctx().scene_detect_objects(data[None], mask=mask[None], back_size=32, segmentation_map=True)
    ref = _ctx().scene_detect(data[None], mask=mask[None], back_size=32, return_maps=True)
    _same_bits(got, ref, SHARED)
    _compare(got, 0, exp, obj, _v(data, ref["back"][0], np.where(mask, 0.0, 1.0)))


def _multiband_case():
    fields, _ = mo.scene()                                    # seed 11
    planes = mo.variance_planes()
    planes[40:42, 32:34, :] = 0.0                             # a defect beside the r_only source
    return fields, planes, dict(noise="absolute", thresh=mo.THRESH, back_size=mo.BACK_SIZE)


def test_multiband_scene_with_a_defect():
    fields, planes, kw = _multiband_case()
    for sel in (None, [2, 4, 0]):
        p = planes if sel is None else planes[:, :, sel]
        exp, obj, details = oo.detect_multiband(fields, bands=sel, planes=p, **kw)
        oo.check_p3_p4(details)
        if sel is None:
            assert (obj["flag"] & oo.MASKED).any() and not (obj["flag"] & oo.MASKED).all()
        got = _ctx().scene_detect_objects(fields[None], bands=sel, weights=p[None], segmentation_map=True, **kw)
        ref = _ctx().scene_detect_multiband(fields[None], bands=sel, weights=p[None], return_maps=True, **kw)
        _same_bits(got, ref, SHARED)
        _compare(got, 0, exp, obj, ref["V"][0])
    # without planes: every pixel counts and bit 8 is never set
    got = _ctx().scene_detect_objects(fields[None], thresh=mo.THRESH, back_size=mo.BACK_SIZE, segmentation_map=True)
    ref = _ctx().scene_detect_multiband(fields[None], thresh=mo.THRESH, back_size=mo.BACK_SIZE, return_maps=True)
    exp, obj, details = oo.detect_multiband(fields, thresh=mo.THRESH, back_size=mo.BACK_SIZE)
    oo.check_p3_p4(details)
    _compare(got, 0, exp, obj, ref["V"][0])
    assert len(got["x"]) > 0 and not (got["flag"] & 8).any()


ROWS = CAT[1:] + INT + DBL + DERIVED


def test_numbering_does_not_see_the_chunks():
    import re

    from debvader_amd._lib import DvError

    fields = np.stack([ds.oracle(n)[0] for n in ds.BATCH])
    kw = ds.oracle(ds.BATCH[0])[3]
    w = np.ones_like(fields)
    ctx = _ctx()
    a = ctx.scene_detect_objects(fields, weights=w, segmentation_map=True, **kw)
    assert np.diff(a["offsets"]).tolist() == [1426, 0, 1, 1, 25]
    for i, name in enumerate(ds.BATCH):
        _, exp, details, _ = ds.oracle(name)
        _compare(a, i, exp, oo.objects(details, exp["D"], exp["v"], wt=w[i]), exp["v"])
    # one field per launch
    with pytest.raises(DvError, match="workspace") as refused:
        ctx.scene_detect_objects(fields, weights=w, segmentation_map=True, workspace_bytes=1, **kw)
    need = int(re.search(r"needs up to (\d+) bytes", str(refused.value)).group(1))
    b = ctx.scene_detect_objects(fields, weights=w, segmentation_map=True, workspace_bytes=need, **kw)
    _same_bits(a, b, ROWS + ("field", "offsets", "globalrms", "segmap"))
    # the fields reversed
    r = ctx.scene_detect_objects(fields[::-1], weights=w, segmentation_map=True, **kw)
    np.testing.assert_array_equal(r["segmap"][::-1], a["segmap"])
    M = len(fields)
    for i in range(M):
        lo, hi = a["offsets"][i], a["offsets"][i + 1]
        rl, rh = r["offsets"][M - 1 - i], r["offsets"][M - i]
        one = ctx.scene_detect_objects(fields[i:i + 1], weights=w[i:i + 1], segmentation_map=True, **kw)      # each alone
        np.testing.assert_array_equal(one["segmap"][0], a["segmap"][i])
        for k in ROWS:
            np.testing.assert_array_equal(r[k][rl:rh], a[k][lo:hi], err_msg=k)
            np.testing.assert_array_equal(one[k], a[k][lo:hi], err_msg=k)
    # the segmap asks for 4 more bytes per pixel, and only when it is asked for
    with pytest.raises(DvError, match="workspace") as refused:
        ctx.scene_detect_objects(fields, weights=w, workspace_bytes=1, **kw)
    assert need - int(re.search(r"needs up to (\d+) bytes", str(refused.value)).group(1)) == 4 * ds.H * ds.W
    with pytest.raises(DvError, match="workspace") as refused:
        ctx.scene_detect(fields, weights=w, workspace_bytes=1, **kw)
    assert int(re.search(r"needs up to (\d+) bytes", str(refused.value)).group(1)) < need - 4 * ds.H * ds.W


def _raw(fields, cap, names, segmap, thresh=0.5, weights=True):
    """dv_scene_detect_objects on painted fields with unit weights, through ctypes: (status, n, catalogue, object arrays)"""
    from debvader_amd import _lib
    from debvader_amd import engine as E

    M, H, W = fields.shape
    k1 = np.ones((1, 1))
    params = _lib.DvDetectParams(thresh, 1e-5, 1, 64, 64, 3, E._dp(k1), 1, 1, 0)
    cat = {k: np.full(cap, -7, np.int32 if k in ("field", "parent", "npix") else np.float64) for k in CAT}
    arr = {k: np.full(cap, -7, np.int32 if k in INT else np.float64) for k in names}
    if segmap:
        arr["segmap"] = np.full((M, H, W), -7, np.int32)
    ostruct = _lib.DvDetectObjects(**{k: (E._ip(v) if v.dtype == np.int32 else E._dp(v)) for k, v in arr.items()})
    w = np.ones_like(fields)
    wstruct = _lib.DvDetectWeights(E._dp(w), 0, 0)
    n = C.c_int64(-1)
    offsets, grms = np.zeros(M + 1, np.int64), np.zeros(M)
    st = _lib.lib.dv_scene_detect_objects(
        _ctx()._h, E._dp(fields), M, H, W, 0, C.byref(params), cap, C.byref(n), offsets.ctypes.data_as(C.POINTER(C.c_int64)),
        E._dp(grms), *[E._ip(cat[k]) if cat[k].dtype == np.int32 else E._dp(cat[k]) for k in CAT],
        C.byref(wstruct) if weights else None, None, C.byref(ostruct))
    return st, n.value, cat, arr


def test_small_cap_partial_requests_and_refusals():
    from debvader_amd import _lib

    fields = np.ascontiguousarray(np.stack([ds.oracle(n)[0] for n in ("comb_minarea1", "nested_mesas")]))
    before = _ctx().scene_detect(fields, weights=np.ones_like(fields), **ds.oracle("comb_minarea1")[3])
    full = _ctx().scene_detect_objects(fields, weights=np.ones_like(fields), segmentation_map=True,
                                       **ds.oracle("comb_minarea1")[3])
    assert len(full["x"]) == 29
    # a cap that is too small: n_out and the segmap, no rows
    st, n, cat, arr = _raw(fields, 5, INT + DBL, True)
    assert st == 0 and n == 29
    np.testing.assert_array_equal(arr["segmap"], full["segmap"])
    assert all((v == -7).all() for v in cat.values()) and all((arr[k] == -7).all() for k in INT + DBL)
    st, n, cat, arr = _raw(fields, n, INT + DBL, True)
    assert st == 0 and n == 29
    for k in CAT + INT + DBL + ("segmap",):
        np.testing.assert_array_equal(arr[k] if k in arr else cat[k], full[k], err_msg=k)
    # the segmap alone; the columns alone; two columns alone
    st, n, cat, arr = _raw(fields, 64, (), True)
    assert st == 0 and list(arr) == ["segmap"]
    np.testing.assert_array_equal(arr["segmap"], full["segmap"])
    _same_bits(_ctx().scene_detect_objects(fields, weights=np.ones_like(fields), segmentation_map=True, columns=False,
                                           **ds.oracle("comb_minarea1")[3]), full, CAT + ("segmap",))
    st, n, cat, arr = _raw(fields, 64, INT + DBL, False)
    assert st == 0 and "segmap" not in arr
    for k in INT + DBL:
        np.testing.assert_array_equal(arr[k][:29], full[k], err_msg=k)
        assert (arr[k][29:] == -7).all()
    st, n, cat, arr = _raw(fields, 64, ("flag", "x2"), False)
    assert st == 0
    np.testing.assert_array_equal(arr["flag"][:29], full["flag"])
    np.testing.assert_array_equal(arr["x2"][:29], full["x2"])
    # refusals, before any GPU work
    st, n, cat, arr = _raw(fields, 64, INT + DBL, True, thresh=-0.5, weights=False)
    assert st == -1 and "thresh" in _lib.last_error() and (arr["segmap"] == -7).all() and n == -1
    st, _, _, _ = _raw(fields, 64, INT + DBL, True, thresh=0.0)              # absolute noise: what the weighted call refuses
    assert st == -1 and "sigma" in _lib.last_error()
    obj = _lib.SIGNATURES["dv_scene_detect_objects"][1]
    null = [0 if a in (C.c_int32, C.c_int64) else None for a in obj]
    null[0] = _ctx()._h
    assert _lib.lib.dv_scene_detect_objects(*null) == -1
    # the engine is as usable as before
    after = _ctx().scene_detect(fields, weights=np.ones_like(fields), **ds.oracle("comb_minarea1")[3])
    _same_bits(before, after, SHARED)


def _set_case():
    from tests.test_gpu_fields_batch import _blob_fields

    F = 131
    return _blob_fields(4, F, seed=11), F


def test_field_set_keeps_the_objects_of_its_last_detection():
    from debvader_amd._lib import DvError
    from tests.test_gpu_fields_batch import _case, _net

    net = _net("float32")
    ctx, eng = net._core.ctx, net._core.engine
    fields, F = _set_case()
    fs = eng.open_field_set(fields)
    old = fs.detect()
    assert sorted(old) == sorted(SHARED)
    keys = ROWS + ("segmap",)

    def check(work, active=None, **kw):
        on = np.ones(4, bool) if active is None else active
        got = fs.detect(active=active, **kw)
        ref = ctx.scene_detect_objects(work[on][:, :, :, 2], segmentation_map=True, **kw)
        assert len(ref["x"]) > 0
        _same_bits(ref, got, ROWS)
        np.testing.assert_array_equal(got["segmap"][on], ref["segmap"])
        assert not got["segmap"][~on].any() and got["segmap"].shape == (4, F, F)
        np.testing.assert_array_equal(got["field"], np.nonzero(on)[0][ref["field"]])
        return got

    fs.set_detect_objects(True, segmentation_map=True)
    first = check(fields)
    _same_bits(old, first, SHARED)                            # the catalogue is the one it was
    assert set(first) == set(SHARED) | set(keys)
    check(fields, active=np.array([True, False, True, True]), thresh=3.0)
    # after one pass: the working residual
    starts, places, fp = _case(F, [12, 0, 30, 7], seed=5, hang=False)
    fs.deblend_pass(starts, places, fp, seed=3)
    work = fs.read("work")
    assert not np.array_equal(work, fields)
    check(work)
    # with weights held: bit 8 comes from them
    w = np.full((4, F, F), 400.0)
    w[:, :, 66] = 0.0
    fs.set_detect_weights(w)
    got = fs.detect(back_size=32)
    ref = ctx.scene_detect_objects(work[:, :, :, 2], weights=w, back_size=32, segmentation_map=True)
    _same_bits(ref, got, keys)
    assert (got["flag"] & 8).any() and not (got["flag"] & 8).all()
    fs.set_detect_weights(None)
    with pytest.raises(ValueError):
        fs.detect(thresh=-1.0)
    # columns without the segmap; then off: the old keys, the old bits
    fs.set_detect_objects(True)
    got = fs.detect()
    assert "segmap" not in got and set(got) == set(SHARED) | set(ROWS)
    fs.set_detect_objects(False)
    off = fs.detect()
    assert sorted(off) == sorted(SHARED)
    _same_bits(got, off, SHARED)
    import ctypes

    from debvader_amd import _lib
    empty = _lib.DvDetectObjects()
    assert _lib.lib.dv_field_set_detect_objects_read(fs._h, len(off["x"]), ctypes.byref(empty)) == -1      # the switch is off
    fs.set_detect_objects(True)
    assert _lib.lib.dv_field_set_detect_objects_read(fs._h, len(off["x"]), ctypes.byref(empty)) == -1      # nothing kept yet
    n = len(fs.detect()["x"])
    assert _lib.lib.dv_field_set_detect_objects_read(fs._h, n + 1, ctypes.byref(empty)) == -1              # a wrong count
    assert _lib.lib.dv_field_set_detect_objects_read(fs._h, n, ctypes.byref(empty)) == 0
    seg = np.zeros((4, F, F), np.int32)
    asked = _lib.DvDetectObjects(segmap=seg.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    assert _lib.lib.dv_field_set_detect_objects_read(fs._h, n, ctypes.byref(asked)) == -1                  # no segmap kept
    _same_bits(off, fs.detect(), CAT)
    fs.close()
    with pytest.raises(DvError, match="closed"):
        fs.set_detect_objects(True)


def test_iterative_catalogue_with_detect_shapes():
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch
    from tests.test_gpu_detect_weighted import _loop_case
    from tests.test_gpu_fields_batch import CS, NB
    from tests.test_gpu_iterative_batch import _loop_net

    fields, _ = _loop_case()
    net = _loop_net("float32")

    def loop():
        net._core.seed_counter = 500
        return IterativeDeblendFieldBatch(net, fields, CS, NB)

    plain = loop()
    a = plain.iterative_catalogue()
    for measure in (False, True):
        it = loop()
        b = it.iterative_catalogue(detect_shapes=True, measure=measure)
        base = a if not measure else loop().iterative_catalogue(measure=True)
        det = [n for n, _ in IterativeDeblendFieldBatch.DETECT_COLUMNS]
        for x, y in zip(base, b):
            assert list(y.dtype.names) == list(x.dtype.names) + det and len(x) == len(y) > 0
            for name in x.dtype.names:
                assert all(np.array_equal(p, q, equal_nan=True) for p, q in zip(x[name], y[name])), name
        assert it.mse == plain.mse
        np.testing.assert_array_equal(it.get_residual_fields(), plain.get_residual_fields())
    # pass 0: the rows of scene_detect_objects on the fields as given, selected by list_idx (the `kept` of batch_windows)
    ref = _ctx().scene_detect_objects(fields[:, :, :, 2])
    for m in range(2):
        first = b[m][b[m]["iteration"] == 0]
        rows = ref["offsets"][m] + first["list_idx"]
        for name in det:
            np.testing.assert_array_equal(first[name], ref[name[4:]][rows], err_msg=name)
        F = fields.shape[1]
        np.testing.assert_array_equal(first["galaxy_distances_to_center_y"], np.round(-int(F / 2) + first["det_x"]))
    # every later pass too: the detection the row's window was cut for
    for m in range(2):
        r = b[m]
        F = fields.shape[1]
        np.testing.assert_array_equal(r["galaxy_distances_to_center_x"], np.round(-int(F / 2) + r["det_y"]))
        assert (r["det_npix"] >= 4).all() and (r["det_xmin"] <= r["det_xmax"]).all()
