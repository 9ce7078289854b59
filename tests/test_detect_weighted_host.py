"""CPU checks of source detection with a per-pixel noise map and a mask: the numpy restatement
(tests/detect_weighted_oracle.py) against the unweighted one and on the 96 x 120 scene of the section, the fill rule of the bad
meshes, the Python argument checks, the keyword plumbing of IterativeDeblendFieldBatch.iterative_catalogue on a stand-in for
the resident set, and the C ABI of the two new calls.  No GPU is touched."""
import inspect
import os
import re

import numpy as np
import pytest

from tests import detect_oracle as do
from tests import detect_weighted_oracle as wo
from tests import test_iterative_batch_host as bh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = [dict(noise="absolute", filter_type="conv", thresh=1.5), dict(noise="absolute", filter_type="conv", thresh=3.0),
            dict(noise="absolute", filter_type="matched", thresh=5.0), dict(noise="relative", filter_type="conv", thresh=1.5)]


def _gauss(shape, cy, cx, sig, amp):
    y, x = np.mgrid[:shape[0], :shape[1]]
    return amp * np.exp(-0.5 * ((x - cx) ** 2 + (y - cy) ** 2) / sig ** 2)


def test_unit_weights_have_the_bits_of_the_unweighted_oracle():
    rng = np.random.default_rng(3)
    f = 100.0 + rng.normal(0, 1.0, (90, 130))
    for cy, cx, a in ((30, 30, 30.0), (30, 36, 20.0), (60, 100, 25.0), (88, 129, 40.0)):
        f += _gauss(f.shape, cy, cx, 2.0, a)
    kern = np.outer([1.0, 2.0, 1.0], [1.0, 3.0, 4.0, 3.0, 1.0])
    for kw in (dict(back_size=32), dict(back_size=64, filter_kernel=kern, minarea=6, nthresh=32, cont=1e-3)):
        ref = do.detect(f, thresh=1.5, **kw)
        assert len(ref["x"]) >= 3
        rel = wo.detect(f, np.ones_like(f), noise="relative", thresh=1.5, **kw)
        # thresh' = thresh * globalrms, the product formed in float64 on the host
        ab = wo.detect(f, np.ones_like(f), noise="absolute", thresh=1.5 * ref["globalrms"], **kw)
        for got in (rel, ab):
            assert got["bad_meshes"] == 0
            for k in ref:
                np.testing.assert_array_equal(got[k], ref[k], err_msg=k)


def test_scene_with_defects_gives_exactly_the_planted_sources():
    data, weights, mask, planted = wo.scene()
    assert np.isnan(data).sum() == 70 and mask[64:96, 64:96].sum() == 24 * 32
    for kw in SETTINGS:
        w = np.where(mask, 0.0, 1.0) if kw["noise"] == "relative" else weights       # relative: a mask only
        r = wo.detect(data, w, back_size=32, **kw)
        assert r["bad_meshes"] == 1, kw
        assert len(r["x"]) == len(planted) == 6, (kw, len(r["x"]))
        d = np.hypot(planted[:, 0][:, None] - r["y"][None], planted[:, 1][:, None] - r["x"][None])
        assert (d.min(axis=1) <= 1.0).all() and sorted(d.argmin(axis=1)) == list(range(6)), kw
        assert np.isneginf(r["D"][mask]).all() and (r["labels"][mask] == -1).all()
    # the unweighted detector on the same pixels, the NaN set to 0: the bleed column is an object of its own
    u = do.detect(np.nan_to_num(data, nan=0.0), back_size=32)
    on_column = np.abs(u["x"] - 52.0) < 1.0
    assert len(u["x"]) == 7 and on_column.sum() == 1 and u["npix"][on_column][0] > 500
    assert u["npix"].max() > 1000                       # the blob around the saturated mesh, the source at (75, 100) in it


def test_masked_values_reach_no_sum():
    data, weights, mask, _ = wo.scene()
    ref = wo.detect(data, weights, back_size=32)
    for val in (np.nan, np.inf, -np.inf, 1e300):
        d = data.copy()
        d[mask] = val
        got = wo.detect(d, weights, back_size=32)
        for k in ref:
            np.testing.assert_array_equal(got[k], ref[k], err_msg=f"{k} under {val}")


def test_bad_mesh_takes_the_mean_of_the_nearest_good_meshes_ties_in_raster_order():
    g = np.array([[np.nan, 2.0, 7.0], [4.0, np.nan, 1.0], [5.0, 3.0, np.nan]])
    good = ~np.isnan(g)
    out = wo.fill_bad(g, good)
    assert out[0, 0] == (2.0 + 4.0) / 2                  # a bad corner: two good meshes at distance 1
    assert out[1, 1] == (((2.0 + 4.0) + 1.0) + 3.0) / 4  # four at distance 1, added in raster order
    assert out[2, 2] == (1.0 + 3.0) / 2
    np.testing.assert_array_equal(out[good], g[good])
    # the order of the sum is the raster order, not the order of the values
    h = np.array([[np.nan, 1e16], [1.0, -1e16]])
    assert wo.fill_bad(h, ~np.isnan(h))[0, 0] == (1e16 + 1.0) / 2
    assert np.isnan(wo.fill_bad(np.full((2, 2), np.nan), np.zeros((2, 2), bool))).all()
    # through the background: a 64 x 64 field of 32-px meshes with the top left mesh masked
    rng = np.random.default_rng(5)
    data = rng.normal(0, 1, (64, 64)) + np.repeat(np.repeat(np.array([[0.0, 10.0], [20.0, 40.0]]), 32, 0), 32, 1)
    w = np.ones((64, 64))
    w[:32, :20] = 0.0                                    # 20 of 32 columns: bad
    bk = wo.background(data, w, bs=32, fs=1)
    assert bk["bad_meshes"] == 1
    b01, _ = do.mesh_stats(data[:32, 32:])
    b10, _ = do.mesh_stats(data[32:, :32])
    assert bk["mesh_back"][0, 0] == (b01 + b10) / 2
    # exactly half counting is good
    w2 = np.ones((64, 64))
    w2[:16, :32] = np.inf
    assert wo.background(data, w2, bs=32, fs=1)["bad_meshes"] == 0
    w2[16, 0] = np.nan
    assert wo.background(data, w2, bs=32, fs=1)["bad_meshes"] == 1


def test_a_field_without_a_good_mesh_has_no_objects():
    data, weights, _, _ = wo.scene()
    r = wo.detect(data, np.zeros_like(weights), back_size=32)
    assert len(r["x"]) == 0 and np.isnan(r["globalrms"]) and (r["labels"] == -1).all() and r["bad_meshes"] == 12


def test_python_argument_checks_fail_before_the_gpu():
    from debvader_amd import engine as E

    shape = (2, 8, 9)
    w = np.ones(shape)
    m = np.zeros(shape, bool)
    m[0, 1, 2] = True
    out, noise, filt = E.check_detect_weights(shape, w, None, None, "conv", 1.5)
    assert noise == 0 and filt == 0 and out.dtype == np.float64
    out, noise, filt = E.check_detect_weights(shape, None, m, None, "matched", 1.5)
    assert noise == 1 and filt == 1 and out[0, 1, 2] == 0.0 and out.sum() == out.size - 1     # a mask alone: relative
    out, noise, _ = E.check_detect_weights(shape, 2.0 * w, m, None, "conv", 1.5)
    assert noise == 0 and out[0, 1, 2] == 0.0 and out[1, 1, 2] == 2.0 and w[0, 1, 2] == 1.0   # (the caller's array is kept)
    assert E.check_detect_weights(shape, w, None, "relative", "conv", -1.0)[1] == 1           # thresh is free when relative
    for bad in (dict(weights=np.ones((2, 8, 8))), dict(mask=np.zeros(shape, np.uint8)), dict(mask=np.zeros((2, 8, 8), bool)),
                dict(noise="poisson"), dict(filter_type="wiener"), dict(thresh=0.0), dict(thresh=-1.5),
                dict(weights=None, mask=None)):
        kw = {**dict(weights=w, mask=None, noise=None, filter_type="conv", thresh=1.5), **bad}
        with pytest.raises(ValueError):
            E.check_detect_weights(shape, kw["weights"], kw["mask"], kw["noise"], kw["filter_type"], kw["thresh"])
    # finite data are required only where the pixel counts
    base = dict(thresh=1.5, minarea=4, nthresh=64, cont=1e-5, filter_kernel=None, back_size=64, back_filter=3)
    f = np.zeros(shape)
    f[0, 1, 2] = np.nan
    ww = w.copy()
    ww[0, 1, 2] = 0.0
    assert E.check_detect_args(f, weights=ww, **base).shape == shape
    with pytest.raises(ValueError, match="counts"):
        E.check_detect_args(f, weights=w, **base)
    with pytest.raises(ValueError, match="finite"):
        E.check_detect_args(f, **base)
    c = E.counting_pixels(np.array([0.0, -1.0, np.nan, np.inf, 1e-300, 3.0]))
    assert c.tolist() == [False, False, False, False, True, True]
    # the new keywords stand behind the existing ones, with defaults that make the existing call
    names = list(inspect.signature(E.Context.scene_detect).parameters)
    assert names[-4:] == ["weights", "mask", "noise", "filter_type"] and names[:3] == ["self", "fields_r", "thresh"]
    sig = inspect.signature(E.Context.scene_detect).parameters
    assert sig["weights"].default is None and sig["mask"].default is None and sig["noise"].default is None
    assert sig["filter_type"].default == "conv"
    assert list(inspect.signature(E.FieldSet.set_detect_weights).parameters)[:4] == ["self", "weights", "noise", "filter_type"]


def test_detect_objects_cuts_band_two_from_four_dimensional_planes():
    from debvader_amd.detect import detection

    class Ctx:
        def scene_detect(self, r_band, **kw):
            self.kw, self.shape = kw, r_band.shape
            return dict(x=np.array([3.2]), y=np.array([4.6]), offsets=np.array([0, 1, 1]))

    img = np.zeros((2, 8, 8, 3))
    w = np.arange(2 * 8 * 8 * 3, dtype=np.float64).reshape(2, 8, 8, 3)
    ctx = Ctx()
    out = detection.detect_objects_batch(img, ctx=ctx, weights=w, noise="relative")
    assert len(out) == 2 and ctx.kw["noise"] == "relative"
    np.testing.assert_array_equal(ctx.kw["weights"], w[:, :, :, 2])
    detection.detect_objects(img, ctx=ctx, mask=np.ones((2, 8, 8), bool), filter_type="matched")
    assert ctx.shape == (1, 8, 8) and ctx.kw["mask"].shape == (1, 8, 8) and ctx.kw["filter_type"] == "matched"
    detection.detect_objects(img, ctx=ctx)
    assert ctx.kw == {}


class WeightedSet(bh.ScriptedSet):
    """tests/test_iterative_batch_host.py's stand-in for the resident set, with the weighted detector's two entry points"""

    def set_detect_weights(self, weights, noise=None, filter_type="conv"):
        self.owner.calls.append(("set_detect_weights", np.array(weights), noise, filter_type))

    def detect(self, active=None, **kw):
        self.owner.calls.append(("detect_kw", dict(kw)))
        return super().detect(active=active)


class WeightedEngine(bh.StubEngine):
    def open_field_set(self, fields, cumulative=False):
        self.calls.append(("open", bool(cumulative)))
        self.sets.append(WeightedSet(self, np.asarray(fields), cumulative))
        return self.sets[-1]


def _batch(script):
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch

    net = bh.Net(script)
    net._core.engine = WeightedEngine(script)
    fields = np.random.default_rng(1).normal(size=(len(script), bh.F, bh.F, bh.NB))
    return IterativeDeblendFieldBatch(net, fields, bh.CS, bh.NB), net._core.engine


def test_iterative_catalogue_sets_the_planes_before_the_first_pass():
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch

    script = [[(3, 0), (4, 0), (2, 0)], [(2, 0), (1, 0)]]
    w4 = np.random.default_rng(2).uniform(0.5, 2.0, (2, bh.F, bh.F, bh.NB))
    w4[0, :, 7, :] = 0.0
    obj, eng = _batch(script)
    res = obj.iterative_catalogue(detect_weights=w4, detect_filter="matched", detect_thresh=4.0)
    names = [c[0] for c in eng.calls]
    assert names.count("set_detect_weights") == 1
    assert names.index("open") < names.index("set_detect_weights") < names.index("detect_kw")
    call = eng.calls[names.index("set_detect_weights")]
    np.testing.assert_array_equal(call[1], w4[:, :, :, 2])             # band 2 of four-dimensional weights
    assert call[2] is None and call[3] == "matched"
    assert all(c[1] == {"thresh": 4.0} for c in eng.calls if c[0] == "detect_kw")
    assert [len(r) for r in res] == [9, 3]                             # 3 + 4 + 2 and 2 + 1: the reference's stopping rule
    # three-dimensional planes pass as they are; noise is handed on
    obj, eng = _batch(script)
    obj.iterative_catalogue(detect_weights=w4[:, :, :, 2], detect_noise="relative")
    call = [c for c in eng.calls if c[0] == "set_detect_weights"][0]
    np.testing.assert_array_equal(call[1], w4[:, :, :, 2])
    assert call[2] == "relative" and call[3] == "conv"
    assert all(c[1] == {} for c in eng.calls if c[0] == "detect_kw")
    # without weights: the calls of the loop as it was, on the unchanged stand-in (its detect takes `active` alone)
    plain, ref, core = bh._run(script)
    obj, eng = _batch(script)
    same = obj.iterative_catalogue()
    assert "set_detect_weights" not in [c[0] for c in eng.calls]
    assert [c[0] for c in eng.calls if c[0] != "detect_kw"] == [c[0] for c in core.engine.calls]
    for a, b in zip(same, ref):
        assert a.dtype == b.dtype and len(a) == len(b)
        for name in a.dtype.names:                       # (object columns hold arrays: compared element by element)
            assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a[name], b[name])), name
    # refusals, before the set is opened
    for bad in (dict(detect_noise="relative"), dict(detect_filter="matched"), dict(detect_weights=np.ones((2, 5, 5))),
                dict(detect_weights=w4, detect_noise="poisson"), dict(detect_weights=w4, detect_filter="wiener"),
                dict(detect_weights=w4, detect_thresh=0.0)):
        obj, eng = _batch(script)
        with pytest.raises(ValueError):
            obj.iterative_catalogue(**bad)
        assert eng.calls == []
    # iterative_deblending keeps the reference's parameter list
    assert list(inspect.signature(IterativeDeblendFieldBatch.iterative_deblending).parameters) == [
        "self", "mse_criterion", "mode", "max_iterations"]
    names = list(inspect.signature(IterativeDeblendFieldBatch.iterative_catalogue).parameters)
    assert names[-5:] == ["detect_weights", "detect_noise", "detect_filter", "detect_thresh", "fit_groups"]


def test_header_export_map_and_ctypes_signatures():
    import ctypes as C

    from debvader_amd import _lib

    header = open(os.path.join(ROOT, "include", "debvader_hip.h")).read()
    assert re.search(r"typedef struct dv_detect_weights \{\s*const double\* weights;[^}]*int32_t noise;[^}]*int32_t filter;[^}]*\}"
                     r" dv_detect_weights;", header)
    for name, val in (("NOISE_ABSOLUTE", 0), ("NOISE_RELATIVE", 1), ("FILTER_CONV", 0), ("FILTER_MATCHED", 1)):
        assert re.search(r"#define DV_DETECT_%s %d\b" % (name, val), header), name
    assert _lib.DETECT_NOISE == {"absolute": 0, "relative": 1} and _lib.DETECT_FILTER == {"conv": 0, "matched": 1}
    m = re.search(r"\bint dv_scene_detect_weighted\(dv_ctx\* ctx,([^;]*)\);", header)
    assert m and re.search(r"const dv_detect_weights\* weights,\s*int32_t\* bad_meshes$", m.group(1).strip())
    assert re.search(r"\bint dv_field_set_detect_weights\(dv_field_set\* set, const double\* weights, int32_t noise, "
                     r"int32_t filter\);", header)
    exports = open(os.path.join(ROOT, "debvader_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*dv_\*;", exports) and re.search(r"local:\s*\*;", exports)
    for name in ("dv_scene_detect_weighted", "dv_field_set_detect_weights"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    plain, weighted = _lib.SIGNATURES["dv_scene_detect"], _lib.SIGNATURES["dv_scene_detect_weighted"]
    assert weighted[0] is C.c_int and weighted[1][:len(plain[1])] == plain[1]       # the arguments of dv_scene_detect, plus
    assert weighted[1][len(plain[1]):] == [C.POINTER(_lib.DvDetectWeights), C.POINTER(C.c_int32)]
    assert [f[0] for f in _lib.DvDetectWeights._fields_] == ["weights", "noise", "filter"]
    assert C.sizeof(_lib.DvDetectWeights) == 16
    assert _lib.SIGNATURES["dv_field_set_detect_weights"][1][1:] == [C.POINTER(C.c_double), C.c_int32, C.c_int32]
    # refused by the library itself on null handles, without a GPU
    assert _lib.lib.dv_field_set_detect_weights(None, None, 0, 0) == -1
    assert _lib.lib.dv_scene_detect_weighted(*[0 if a in (C.c_int32, C.c_int64) else None for a in weighted[1]]) == -1
