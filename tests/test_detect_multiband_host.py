"""CPU checks of multi-band source detection: the numpy restatement
(tests/detect_multiband_oracle.py) on the 96 x 120 x 6 scene of the section - what the combination of the bands finds that
band 2 alone does not -, its reductions to the single-band oracles, the rules for bands that do not count, the Python
argument checks, the plumbing of detect_objects, FieldSet.set_detect_bands and iterative_catalogue over stand-ins, and the C
ABI of the two new calls.  No GPU is touched."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest

from tests import detect_multiband_oracle as mo
from tests import detect_oracle as do
from tests import detect_weighted_oracle as wo
from tests import test_iterative_batch_host as bh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(thresh=mo.THRESH, back_size=mo.BACK_SIZE)
FOUND = ("all", "r_only", "not_r", "faint")


@functools.lru_cache(maxsize=None)
def _scene():
    fields, pos = mo.scene()
    fields.setflags(write=False)
    return fields, pos


@functools.lru_cache(maxsize=None)
def _six():
    return mo.detect(_scene()[0], **KW)


@functools.lru_cache(maxsize=None)
def _single(b):
    return mo.detect(_scene()[0], bands=[b], **KW)


def _found(r, pos):
    """the names of the planted sources with a catalogue row within 1 px, and the rows that belong to none"""
    names, used = [], np.zeros(len(r["x"]), bool)
    for name, (row, col) in pos.items():
        d = np.hypot(r["y"] - row, r["x"] - col)
        if len(d) and d.min() <= 1.0:
            names.append(name)
            used[np.argmin(d)] = True
    return tuple(names), int((~used).sum())


def test_the_scene_meets_its_conditions():
    """conditions on the scene (the two faint amplitudes were tuned until they held), asserted before anything is concluded"""
    _, pos = _scene()
    S, T = _six()["D"], mo.THRESH
    for name in FOUND:
        assert S[mo.near(pos[name])].max() >= T + 0.5, name
    assert S[mo.near(pos["red"])].max() <= T - 0.4
    far = np.ones(S.shape, bool)
    for p in pos.values():
        far &= ~mo.near(p, radius=12.0)
    assert S[far].max() <= T - 1.0
    assert np.abs(S - T).min() > 1e-9                            # no label sits on a rounding edge
    for b in range(6):                                           # ... and no single band comes near finding "faint"
        Sb = _single(b)["D"]
        assert Sb[mo.near(pos["faint"])].max() <= T - 0.4, b
        assert np.abs(Sb - T).min() > 1e-9
    Sr = _single(2)["D"]
    assert Sr[mo.near(pos["not_r"])].max() <= T - 0.4 and Sr[mo.near(pos["r_only"])].max() >= T + 0.5


def test_six_bands_find_what_band_two_alone_does_not():
    _, pos = _scene()
    assert _found(_six(), pos) == (FOUND, 0)
    assert _found(_single(2), pos) == (("all", "r_only"), 0)
    for b in range(6):
        assert "faint" not in _found(_single(b), pos)[0], b


def test_band_weights_match_the_combination_to_a_red_source():
    fields, pos = _scene()
    red = mo.near(pos["red"])
    flat = _six()["D"][red].max()
    shaped = mo.detect(fields, band_weights=mo.RED_WEIGHTS, **KW)
    assert shaped["D"][red].max() >= 1.3 * flat
    # scaling c scales V and leaves S where it was, up to rounding
    twice = mo.detect(fields, band_weights=[2.0 * c for c in mo.RED_WEIGHTS], **KW)
    np.testing.assert_allclose(twice["D"], shaped["D"], rtol=1e-12)
    np.testing.assert_allclose(twice["V"], shaped["V"] / 2.0, rtol=1e-12, atol=1e-300)


def test_one_band_reduces_to_the_weighted_oracle():
    fields, _ = _scene()
    for b in (2, 4):
        got = _single(b)
        plain = do.background(fields[:, :, b], mo.BACK_SIZE, 3)
        w = 1.0 / (plain["rms"] * plain["rms"])
        ref = wo.detect(fields[:, :, b], w, noise="absolute", **KW)
        for key in ("D", "labels") + do.CAT_KEYS:
            np.testing.assert_array_equal(got[key], ref[key], err_msg=key)
        np.testing.assert_array_equal(got["V"], ref["v"])
        np.testing.assert_array_equal(got["Wt"], w)
        np.testing.assert_array_equal(got["back"][:, :, 0], plain["back"])
        np.testing.assert_array_equal(got["rms"][:, :, 0], plain["rms"])
        assert got["globalrms"] == 1.0 / np.sqrt(1.0 / (plain["globalrms"] * plain["globalrms"]))
        assert got["band_globalrms"][0] == plain["globalrms"] and len(ref["x"]) >= 2


def test_unit_relative_planes_equal_no_planes():
    fields, _ = _scene()
    ones = np.ones(fields.shape)
    a = mo.detect(fields, planes=ones, noise="relative", **KW)
    for key, val in _six().items():
        np.testing.assert_array_equal(a[key], val, err_msg=key)
    sel = mo.detect(fields, bands=[4, 0], planes=ones[:, :, :2], noise="relative", band_weights=[1.0, 0.5], **KW)
    ref = mo.detect(fields, bands=[4, 0], band_weights=[1.0, 0.5], **KW)
    for key, val in ref.items():
        np.testing.assert_array_equal(sel[key], val, err_msg=key)


def test_a_band_masked_at_a_pixel_leaves_the_sums_and_the_rest_counts():
    fields, _ = _scene()
    P = mo.variance_planes()
    ref = mo.combine(fields, planes=P, noise="absolute", back_size=mo.BACK_SIZE)
    f, Q = fields.copy(), P.copy()
    Q[10:14, 50:58, 3] = 0.0                                     # a NaN block under a mask, in band 3 only
    f[10:14, 50:58, 3] = np.nan
    Q[60:64, 5:9, :] = 0.0                                       # masked in all bands
    f[60:64, 5:9, :] = np.inf
    got = mo.combine(f, planes=Q, noise="absolute", back_size=mo.BACK_SIZE)
    blk = (slice(10, 14), slice(50, 58))
    assert got["counts"][blk][..., [0, 1, 2, 4, 5]].all() and not got["counts"][blk][..., 3].any()
    np.testing.assert_allclose(ref["Wt"][blk] - got["Wt"][blk], P[blk][..., 3], rtol=1e-12)       # Wt drops by that band's term
    assert np.isfinite(got["V"]).all() and (got["Wt"][60:64, 5:9] == 0).all() and (got["V"][60:64, 5:9] == 0).all()
    r = mo.detect(f, planes=Q, noise="absolute", **KW)
    assert np.isneginf(r["D"][60:64, 5:9]).all() and np.isfinite(r["D"][blk]).all() and (r["labels"][60:64, 5:9] == -1).all()
    for val in (np.nan, -np.inf, 1e300):                        # what lies under a band that does not count reaches nothing
        g = f.copy()
        g[10:14, 50:58, 3] = val
        g[60:64, 5:9, :] = val
        again = mo.detect(g, planes=Q, noise="absolute", **KW)
        for key, v in r.items():
            np.testing.assert_array_equal(again[key], v, err_msg=f"{key} under {val}")


def test_a_band_without_a_good_mesh_is_ignored_and_a_field_without_a_good_band_is_empty():
    fields, pos = _scene()
    P = mo.variance_planes()
    Q = P.copy()
    Q[:, :, 5] = 0.0
    Q[40:60, 40:52, 5] = 1.0                                     # 240 counting pixels: under half of the mesh they lie in
    f = fields.copy()
    f[:30, :, 5] = np.nan
    got = mo.detect(f, planes=Q, noise="absolute", **KW)
    five = mo.detect(fields, bands=[0, 1, 2, 3, 4], planes=P[:, :, :5], noise="absolute", **KW)
    assert got["bad_meshes"].tolist() == [0, 0, 0, 0, 0, 12] and not got["counts"][:, :, 5].any()
    assert np.isnan(got["band_globalrms"][5]) and got["globalrms"] == five["globalrms"]
    for key in ("V", "Wt", "D", "labels") + do.CAT_KEYS:
        np.testing.assert_array_equal(got[key], five[key], err_msg=key)
    assert "faint" in _found(got, pos)[0]
    none = mo.detect(f, planes=np.zeros_like(P), noise="absolute", **KW)
    assert len(none["x"]) == 0 and np.isnan(none["globalrms"]) and (none["labels"] == -1).all()
    assert none["bad_meshes"].tolist() == [12] * 6 and np.isneginf(none["D"]).all() and not none["V"].any()


def test_one_counting_band_with_a_band_weight_is_v_over_c():
    fields, _ = _scene()
    P = mo.variance_planes()[:, :, :2].copy()
    P[20:30, 20:40, 0] = 0.0                                     # there only band 1 counts
    got = mo.combine(fields, bands=[0, 1], band_weights=[1.0, 4.0], planes=P, noise="absolute", back_size=mo.BACK_SIZE)
    blk = (slice(20, 30), slice(20, 40))
    v1 = fields[:, :, 1] - got["back"][:, :, 1]
    np.testing.assert_array_equal(got["V"][blk], (v1 / 4.0)[blk])
    np.testing.assert_array_equal(got["Wt"][blk], (16.0 * P[:, :, 1])[blk])
    out = (slice(40, 50), slice(20, 40))
    v0 = fields[:, :, 0] - got["back"][:, :, 0]
    w0, w1 = P[:, :, 0], P[:, :, 1]
    np.testing.assert_array_equal(got["V"][out], (((1.0 * w0) * v0 + (4.0 * w1) * v1) / (1.0 * w0 + 16.0 * w1))[out])


BAD_ARGS = [dict(bands=[]), dict(bands=[0, 1, 2, 3, 4, 5, 0]), dict(bands=[6]), dict(bands=[-1]), dict(bands=[1, 1]),
            dict(band_weights=[1.0] * 5), dict(band_weights=[1, 1, 1, 1, 1, 0.0]), dict(band_weights=[1, 1, 1, 1, 1, np.inf]),
            dict(band_weights=[1, 1, 1, 1, 1, np.nan]), dict(band_weights=[1, 1, 1, 1, 1, -2.0]), dict(thresh=0.0),
            dict(thresh=-1.0), dict(filter_type="wiener"), dict(noise="relative")]


def test_every_refusal_of_the_oracle_and_of_the_python_checks():
    from debvader_amd import engine as E

    fields, _ = _scene()
    small = fields[:8, :9]
    for bad in BAD_ARGS:
        with pytest.raises(ValueError):
            mo.detect(small, **{**KW, **bad})
    with pytest.raises(ValueError):
        mo.detect(small, planes=np.ones(small.shape), noise="poisson", **KW)
    # the Python checks of the engine, before any GPU work
    sel, c = E.check_detect_bands(6, None, None)
    assert sel.tolist() == list(range(6)) and sel.dtype == np.int32 and c.tolist() == [1.0] * 6
    sel, c = E.check_detect_bands(6, range(6), None)
    assert sel.tolist() == list(range(6))
    sel, c = E.check_detect_bands(3, (2, 0), (1, 0.5))
    assert sel.tolist() == [2, 0] and c.tolist() == [1.0, 0.5] and c.dtype == np.float64
    for bad in BAD_ARGS[:10] + [dict(bands=[0.5]), dict(bands=[[0, 1]])]:
        with pytest.raises(ValueError):
            E.check_detect_bands(6, bad.get("bands"), bad.get("band_weights"))
    shape = (2, 8, 9, 3)
    w = np.ones(shape)
    m3 = np.zeros(shape[:3], bool)
    m3[0, 1, 2] = True
    assert E.check_detect_band_planes(shape, None, None, None, "matched", 1.5) == (None, 0, 1)
    p, noise, filt = E.check_detect_band_planes(shape, 2.0 * w, m3, None, "conv", 1.5)
    assert noise == 0 and filt == 0 and (p[0, 1, 2] == 0).all() and p[1, 1, 2, 0] == 2.0 and p.shape == shape
    m4 = np.zeros(shape, bool)
    m4[1, 0, 0, 2] = True
    p, noise, _ = E.check_detect_band_planes(shape, None, m4, None, "conv", 1.5)
    assert noise == 1 and p.sum() == p.size - 1 and p[1, 0, 0, 2] == 0                        # a mask alone: relative
    for bad in (dict(weights=np.ones((2, 8, 9))), dict(weights=np.ones((2, 8, 9, 6))), dict(mask=np.zeros((2, 8, 8), bool)),
                dict(mask=np.zeros(shape, np.uint8)), dict(noise="poisson", weights=w), dict(noise="relative"),
                dict(filter_type="wiener"), dict(thresh=0.0), dict(thresh=-2.0, weights=w, noise="relative")):
        kw = {**dict(weights=None, mask=None, noise=None, filter_type="conv", thresh=1.5), **bad}
        with pytest.raises(ValueError):
            E.check_detect_band_planes(shape, kw["weights"], kw["mask"], kw["noise"], kw["filter_type"], kw["thresh"])
    # the new method's parameter list; the existing ones keep theirs
    names = list(inspect.signature(E.Context.scene_detect_multiband).parameters)
    assert names == ["self", "fields", "bands", "band_weights", "thresh", "minarea", "nthresh", "cont", "filter_kernel",
                     "back_size", "back_filter", "return_maps", "workspace_bytes", "weights", "mask", "noise", "filter_type"]
    assert list(inspect.signature(E.Context.scene_detect).parameters)[-4:] == ["weights", "mask", "noise", "filter_type"]
    assert list(inspect.signature(E.FieldSet.set_detect_bands).parameters) == [
        "self", "bands", "band_weights", "weights", "mask", "noise", "filter_type"]
    assert list(inspect.signature(E.FieldSet.detect).parameters) == [
        "self", "active", "thresh", "minarea", "nthresh", "cont", "filter_kernel", "back_size", "back_filter", "workspace_bytes"]
    ctx = E.Context.__new__(E.Context)                           # (no handle: every refusal comes before the library)
    for bad in (dict(fields=np.zeros((1, 8, 9))), dict(bands=[7]), dict(band_weights=[1.0]), dict(thresh=0.0),
                dict(weights=np.ones((1, 8, 9))), dict(noise="absolute"), dict(filter_type="wiener"),
                dict(fields=np.full((1, 8, 9, 6), np.nan)), dict(back_size=0), dict(minarea=0)):
        kw = {**dict(fields=np.zeros((1, 8, 9, 6))), **bad}
        with pytest.raises(ValueError):
            ctx.scene_detect_multiband(**kw)
    nanf = np.zeros((1, 8, 9, 6))
    nanf[0, 1, 1, 3] = np.nan
    with pytest.raises(ValueError, match="counts"):
        ctx.scene_detect_multiband(nanf, weights=np.ones((1, 8, 9, 6)))
    with pytest.raises(ValueError, match="finite"):
        ctx.scene_detect_multiband(nanf, bands=[3])


class Ctx:
    def scene_detect(self, r_band, **kw):
        self.single = (r_band.shape, kw)
        return dict(x=np.array([3.2]), y=np.array([4.6]), offsets=np.array([0, 1, 1]))

    def scene_detect_multiband(self, fields, **kw):
        self.multi = (np.shape(fields), kw)
        n = len(fields)                                          # one object per field
        return dict(x=np.array([3.2, 1.0])[:n], y=np.array([4.6, 2.0])[:n], offsets=np.arange(n + 1))


def test_detect_objects_hands_whole_fields_and_indexed_planes_to_the_new_method():
    from debvader_amd.detect import detection

    img = np.zeros((2, 8, 8, 6))
    w = np.arange(2 * 8 * 8 * 6, dtype=np.float64).reshape(2, 8, 8, 6)
    m3 = np.zeros((2, 8, 8), bool)
    ctx = Ctx()
    out = detection.detect_objects_batch(img, ctx=ctx, bands=(4, 0), band_weights=(1.0, 2.0), weights=w, mask=m3, thresh=2.5)
    shape, kw = ctx.multi
    assert shape == (2, 8, 8, 6) and kw["bands"] == (4, 0) and kw["band_weights"] == (1.0, 2.0) and kw["thresh"] == 2.5
    np.testing.assert_array_equal(kw["weights"], w[:, :, :, [4, 0]])
    assert kw["mask"].shape == (2, 8, 8) and len(out) == 2 and out[1].tolist() == [[-2.0, -3.0]]
    one = detection.detect_objects(img, ctx=ctx, bands=None, mask=np.ones((2, 8, 8, 6), bool))
    shape, kw = ctx.multi
    assert shape == (1, 8, 8, 6) and kw["bands"] is None and kw["mask"].shape == (1, 8, 8, 6) and one.shape == (1, 2)
    # without bands: the call as it was, on band 2
    detection.detect_objects(img, ctx=ctx)
    assert ctx.single == ((1, 8, 8), {})
    detection.detect_objects_batch(img, ctx=ctx, weights=w)
    np.testing.assert_array_equal(ctx.single[1]["weights"], w[:, :, :, 2])
    for fn in (detection.detect_objects, detection.detect_objects_batch):
        with pytest.raises(ValueError, match="bands"):
            fn(img, ctx=ctx, band_weights=(1.0,) * 6)
        assert list(inspect.signature(fn).parameters)[:4] == ["field_image" if fn is detection.detect_objects else "field_images",
                                                               "ctx", "bands", "band_weights"]


class BandsSet(bh.ScriptedSet):
    """tests/test_iterative_batch_host.py's stand-in for the resident set, with the detector's entry points"""

    def set_detect_bands(self, bands, band_weights=None, weights=None, mask=None, noise=None, filter_type="conv"):
        self.owner.calls.append(("set_detect_bands", np.array(bands), band_weights, weights, mask, noise, filter_type))

    def set_detect_weights(self, weights, noise=None, filter_type="conv"):
        self.owner.calls.append(("set_detect_weights",))

    def detect(self, active=None, **kw):
        self.owner.calls.append(("detect_kw", dict(kw)))
        return super().detect(active=active)


class BandsEngine(bh.StubEngine):
    def open_field_set(self, fields, cumulative=False):
        self.calls.append(("open", bool(cumulative)))
        self.sets.append(BandsSet(self, np.asarray(fields), cumulative))
        return self.sets[-1]


def _batch(script):
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch

    net = bh.Net(script)
    net._core.engine = BandsEngine(script)
    fields = np.random.default_rng(1).normal(size=(len(script), bh.F, bh.F, bh.NB))
    return IterativeDeblendFieldBatch(net, fields, bh.CS, bh.NB), net._core.engine


def test_iterative_catalogue_sets_the_bands_before_the_first_pass():
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch

    script = [[(3, 0), (4, 0), (2, 0)], [(2, 0), (1, 0)]]
    w4 = np.random.default_rng(2).uniform(0.5, 2.0, (2, bh.F, bh.F, bh.NB))
    obj, eng = _batch(script)
    res = obj.iterative_catalogue(detect_bands=range(6), detect_thresh=2.5)
    names = [c[0] for c in eng.calls]
    assert names.count("set_detect_bands") == 1 and "set_detect_weights" not in names
    assert names.index("open") < names.index("set_detect_bands") < names.index("detect_kw")
    call = eng.calls[names.index("set_detect_bands")]
    assert call[1].tolist() == list(range(6)) and call[2].tolist() == [1.0] * 6 and call[3] is None and call[4] is None
    assert call[5] is None and call[6] == "conv"
    assert all(c[1] == {"thresh": 2.5} for c in eng.calls if c[0] == "detect_kw")
    assert [len(r) for r in res] == [9, 3]                       # the reference's stopping rule, as without bands
    # four-dimensional weights give the planes of the selected bands, in their order
    obj, eng = _batch(script)
    obj.iterative_catalogue(detect_bands=(4, 1), detect_band_weights=(1.0, 0.5), detect_weights=w4, detect_noise="relative",
                            detect_filter="matched")
    call = [c for c in eng.calls if c[0] == "set_detect_bands"][0]
    assert call[1].tolist() == [4, 1] and call[2].tolist() == [1.0, 0.5] and call[5] == "relative" and call[6] == "matched"
    np.testing.assert_array_equal(call[3], w4[:, :, :, [4, 1]])
    # the matched filter needs no planes here
    obj, eng = _batch(script)
    obj.iterative_catalogue(detect_bands=[2], detect_filter="matched")
    assert [c for c in eng.calls if c[0] == "set_detect_bands"][0][6] == "matched"
    # refusals, before the set is opened
    with pytest.raises(ValueError, match="plane per band"):
        _batch(script)[0].iterative_catalogue(detect_bands=range(6), detect_weights=w4[:, :, :, 2])
    for bad in (dict(detect_band_weights=(1.0,) * 6), dict(detect_bands=[6]), dict(detect_bands=[0, 0]),
                dict(detect_bands=[0], detect_band_weights=[0.0]), dict(detect_bands=[0], detect_noise="relative"),
                dict(detect_bands=[0], detect_thresh=0.0), dict(detect_bands=[0], detect_filter="wiener"),
                dict(detect_bands=[0, 1], detect_weights=w4[:, :, :, :2])):
        obj, eng = _batch(script)
        with pytest.raises(ValueError):
            obj.iterative_catalogue(**bad)
        assert eng.calls == []
    # without detect_bands: the calls of the loop as it was
    plain, ref, core = bh._run(script)
    obj, eng = _batch(script)
    same = obj.iterative_catalogue()
    assert "set_detect_bands" not in [c[0] for c in eng.calls]
    assert [c[0] for c in eng.calls if c[0] != "detect_kw"] == [c[0] for c in core.engine.calls]
    assert [len(a) for a in same] == [len(b) for b in ref]
    # the parameter lists: the two new keywords in front of fit_groups, which stays last; the reference's list is kept
    params = inspect.signature(IterativeDeblendFieldBatch.iterative_catalogue).parameters
    names = list(params)
    assert names[-1] == "fit_groups" and names.index("detect_bands") + 1 == names.index("detect_band_weights") < len(names) - 1
    assert params["detect_bands"].default is None and params["detect_band_weights"].default is None
    assert list(inspect.signature(IterativeDeblendFieldBatch.iterative_deblending).parameters) == [
        "self", "mse_criterion", "mode", "max_iterations"]


def test_header_export_map_and_ctypes_signatures():
    from debvader_amd import _lib

    header = open(os.path.join(ROOT, "include", "debvader_hip.h")).read()
    assert re.search(r"typedef struct dv_detect_bands \{\s*const int32_t\* bands;[^}]*int32_t k;[^}]*const double\* band_weights;"
                     r"[^}]*const double\* planes;[^}]*int32_t noise;[^}]*int32_t filter;[^}]*\} dv_detect_bands;", header)
    m = re.search(r"\bint dv_scene_detect_multiband\(dv_ctx\* ctx,([^;]*)\);", header)
    assert m and re.search(r"const dv_detect_bands\* bands,\s*double\* band_globalrms,\s*int32_t\* bad_meshes$", m.group(1).strip())
    assert re.search(r"\bint dv_field_set_detect_bands\(dv_field_set\* set, const int32_t\* bands, int32_t k, "
                     r"const double\* band_weights,\s*const double\* planes, int32_t noise, int32_t filter\);", header)
    exports = open(os.path.join(ROOT, "debvader_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*dv_\*;", exports) and re.search(r"local:\s*\*;", exports)
    for name in ("dv_scene_detect_multiband", "dv_field_set_detect_bands"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    plain, multi = _lib.SIGNATURES["dv_scene_detect"][1], _lib.SIGNATURES["dv_scene_detect_multiband"][1]
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    # the arguments of dv_scene_detect with nb behind W, V and Wt between rms and D, and the three new ones at the end
    assert multi[:5] == plain[:5] and multi[5] is C.c_int32 and multi[6:20] == plain[5:19]
    assert multi[20:] == [dp, dp, dp, ip, C.POINTER(_lib.DvDetectBands), dp, ip] and plain[19:] == [dp, ip]
    assert [f[0] for f in _lib.DvDetectBands._fields_] == ["bands", "k", "band_weights", "planes", "noise", "filter"]
    assert C.sizeof(_lib.DvDetectBands) == 40
    assert _lib.SIGNATURES["dv_field_set_detect_bands"][1][1:] == [ip, C.c_int32, dp, dp, C.c_int32, C.c_int32]
    # the argument counts of the existing detector entry points are unchanged
    counts = {name: len(_lib.SIGNATURES[name][1]) for name in ("dv_scene_detect", "dv_scene_detect_weighted",
                                                               "dv_field_set_detect", "dv_field_set_detect_weights")}
    assert counts == {"dv_scene_detect": 21, "dv_scene_detect_weighted": 23, "dv_field_set_detect": 14,
                      "dv_field_set_detect_weights": 4}
    # refused by the library itself on null handles, without a GPU
    assert _lib.lib.dv_field_set_detect_bands(None, None, 0, None, None, 0, 0) == -1
    assert _lib.lib.dv_scene_detect_multiband(*[0 if a in (C.c_int32, C.c_int64) else None for a in multi]) == -1
